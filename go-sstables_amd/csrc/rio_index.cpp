// rio_index.cpp — DiskKeyIndex lookups of librio (include/rio.h): the device-resident batch search and the
// host-memory rio_index handle (k_index_search / k_index_search_view in rio_seek.hip, rio_sort.hip).
#include <algorithm>

#include "rio_ctx.h"

using namespace rio;

extern "C" int rio_device_index_search(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t seek_len,
                                       const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n,
                                       rio_index_hit* d_hits, void* stream) {
    if (!ctx || !d_file || (n && (!d_keys || !d_key_off || !d_hits))) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream_of(ctx, stream);
    const uint32_t* perm = nullptr;
    if (n >= 4096 && n < 0x7FFFFFFFull) {  // big batches: visit the queries in key order (rio_sort.hip)
        rio_ctx::Query& Q = ctx->q;
        const size_t tb = std::max<size_t>(key_sort_tmp_bytes(n), 256);
        HIP_TRY(Q.pfx.ensure(n * 8));
        HIP_TRY(Q.pfx_out.ensure(n * 8));
        HIP_TRY(Q.idx.ensure(n * 4));
        HIP_TRY(Q.perm.ensure(n * 4));
        HIP_TRY(Q.tmp.ensure(tb));
        HIP_TRY(launch_key_sort(d_keys, d_key_off, n, Q.pfx.as<uint64_t>(), Q.pfx_out.as<uint64_t>(),
                                Q.idx.as<uint32_t>(), Q.perm.as<uint32_t>(), Q.tmp.p, Q.tmp.cap, s));
        perm = Q.perm.as<uint32_t>();
    }
    return hip_status(launch_index_search(d_file, len, seek_len ? seek_len : 4096, d_keys, d_key_off, n, perm, d_hits, s));
}

struct rio_index {
    rio_ctx* ctx = nullptr;
    uint64_t len = 0;
    DevBuf file, keys, key_off, hits;
    // a compressed index.rio: its decoded records and SeekNext map (k_index_search_view)
    bool view = false;
    uint64_t n = 0, K = 0;
    DevBuf v_out, v_off, v_rec, v_flags, v_P, v_R;
};

// The view of a compressed index (DiskKeyIndex over rProto.NewMMapProtoReaderWithPath, which decompresses
// every record it reads, sstables/disk_key_index.go:173): the FileReader sequence of records (rio_frame +
// rio_decode on the index's context) and the SeekNext map over the file (build_seek_map), all resident.
static int index_build_view(rio_index* x, const uint8_t* file, uint64_t len) {
    rio_ctx* ctx = x->ctx;
    std::lock_guard<std::mutex> cg(ctx->mu);  // reader handles sharing the context take it around device use
    rio_file_info fi{};
    int rc = rio_frame(ctx, file, len, &fi);
    if (rc) return rc;
    if (nothing_framed(fi.status)) return RIO_OK;  // no view: the kernel reports the header's status per query
    const uint64_t n = fi.n_records, nb = fi.total_out_bytes;
    std::vector<uint8_t> out(nb + 1), flags(n + 1);
    std::vector<uint64_t> off(n + 1), rec(n + 1);
    rc = rio_decode(ctx, out.data(), nb, off.data(), rec.data(), flags.data(), n, &fi);
    if (rc) return rc;
    const uint64_t m = std::min<uint64_t>(fi.n_records, n);
    HIP_TRY(x->v_out.ensure(nb + 16));
    HIP_TRY(x->v_off.ensure((m + 1) * 8));
    HIP_TRY(x->v_rec.ensure((m + 1) * 8));
    HIP_TRY(x->v_flags.ensure(m + 8));
    if (nb) HIP_TRY(hipMemcpyAsync(x->v_out.p, out.data(), nb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(x->v_off.p, off.data(), (m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (m) {
        HIP_TRY(hipMemcpyAsync(x->v_rec.p, rec.data(), m * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(x->v_flags.p, flags.data(), m, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> P, R;
    if (build_seek_map(x->file.as<uint8_t>(), len, x->v_rec.as<uint64_t>(), x->v_flags.as<uint8_t>(), m, P, R,
                       ctx->stream))
        return RIO_ERR_HIP;
    HIP_TRY(x->v_P.ensure(P.size() * 8 + 8));
    HIP_TRY(x->v_R.ensure(R.size() * 8 + 8));
    if (!P.empty()) {
        HIP_TRY(hipMemcpyAsync(x->v_P.p, P.data(), P.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(x->v_R.p, R.data(), R.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    x->n = m;
    x->K = P.size();
    x->view = true;
    return RIO_OK;
}

extern "C" int rio_index_open(rio_ctx* ctx, const uint8_t* file, uint64_t len, rio_index** out) {
    if (!ctx || !out || (!file && len)) return RIO_ERR_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    auto* x = new rio_index();
    x->ctx = ctx;
    x->len = len;
    int rc = x->file.ensure(len + RIO_DEVICE_PAD) ? RIO_ERR_HIP : RIO_OK;
    if (!rc) rc = h2d_staged(ctx, x->file.p, file, len);
    if (!rc && hipMemsetAsync(x->file.as<uint8_t>() + len, 0, RIO_DEVICE_PAD, ctx->stream) != hipSuccess) rc = RIO_ERR_HIP;
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = RIO_ERR_HIP;
    if (!rc && len >= RIO_FILE_HEADER_BYTES) {
        const uint32_t v = file[0] | (uint32_t)file[1] << 8 | (uint32_t)file[2] << 16 | (uint32_t)file[3] << 24;
        const uint32_t c = file[4] | (uint32_t)file[5] << 8 | (uint32_t)file[6] << 16 | (uint32_t)file[7] << 24;
        if (v >= RIO_VERSION1 && v <= RIO_VERSION4 && c != RIO_COMP_NONE && c <= RIO_COMP_LZW) rc = index_build_view(x, file, len);
    }
    if (rc) {
        delete x;
        return rc;
    }
    *out = x;
    return RIO_OK;
}

extern "C" int rio_index_search(rio_index* x, const uint8_t* keys, const uint64_t* key_off, uint64_t n,
                                rio_index_hit* hits) {
    if (!x || (n && (!key_off || !hits))) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    rio_ctx* ctx = x->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t kb = key_off[n];
    if (kb && !keys) return RIO_ERR_ARG;
    HIP_TRY(x->keys.ensure(kb + 16));
    HIP_TRY(x->key_off.ensure((n + 1) * 8));
    HIP_TRY(x->hits.ensure(n * sizeof(rio_index_hit)));
    int rc = kb ? h2d_staged(ctx, x->keys.p, keys, kb) : RIO_OK;
    if (!rc) rc = h2d_staged(ctx, x->key_off.p, reinterpret_cast<const uint8_t*>(key_off), (n + 1) * 8);
    if (rc) return rc;
    if (x->view) {
        HIP_TRY(launch_index_search_view(x->v_out.as<uint8_t>(), x->v_off.as<uint64_t>(), x->v_flags.as<uint8_t>(), x->n,
                                         x->v_P.as<uint64_t>(), x->K, x->v_R.as<uint64_t>(), x->len, x->keys.as<uint8_t>(),
                                         x->key_off.as<uint64_t>(), n, nullptr, x->hits.as<rio_index_hit>(), ctx->stream));
    } else {
        rc = rio_device_index_search(ctx, x->file.as<uint8_t>(), x->len, 4096, x->keys.as<uint8_t>(),
                                     x->key_off.as<uint64_t>(), n, x->hits.as<rio_index_hit>(), nullptr);
        if (rc) return rc;
    }
    return d2h_staged(ctx, reinterpret_cast<uint8_t*>(hits), x->hits.p, n * sizeof(rio_index_hit));
}

// the handle's arenas free themselves: as for a context, only after the work on them has completed
extern "C" void rio_index_free(rio_index* x) {
    if (!x) return;
    hipSetDevice(x->ctx->device);
    hipStreamSynchronize(x->ctx->stream);
    delete x;
}
