// rio_encoder.cpp — recordio v4 encoding entry points of librio (include/rio.h; kernels in rio_encode.hip).
#include <algorithm>

#include "rio_ctx.h"

using namespace rio;

extern "C" uint64_t rio_encode_bound(uint64_t n, uint64_t total_bytes, uint32_t compression) {
    const uint64_t payload = compression == RIO_COMP_SNAPPY ? 32 * n + total_bytes + total_bytes / 6 : total_bytes;
    return RIO_FILE_HEADER_BYTES + RIO_RECORD_HEADER_V4_MAX * n + payload + 64;
}

extern "C" int rio_device_encode(rio_ctx* ctx, const uint8_t* d_records, const uint64_t* d_rec_off,
                                 const uint8_t* d_flags, uint64_t n, uint64_t total_bytes, uint32_t compression,
                                 uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_rec_off, uint64_t* d_out_len,
                                 void* stream) {
    if (!ctx || !d_rec_off || !d_out || !d_out_len || (n && (!d_records || !d_out_rec_off))) return RIO_ERR_ARG;
    if (compression != RIO_COMP_NONE && compression != RIO_COMP_SNAPPY) return RIO_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::Encode& E = ctx->enc;
    const size_t cub = std::max<size_t>(enc_cub_bytes(n), 256);
    HIP_TRY(E.scr.ensure(enc_scratch_bytes(n, total_bytes, compression)));
    HIP_TRY(E.scr_off.ensure((n + 1) * 8));
    HIP_TRY(E.clen.ensure(n * 8 + 8));
    // per-lane global hash tables only when some record can exceed the LDS kernel's 1 KiB
    if (compression == RIO_COMP_SNAPPY) HIP_TRY(E.tab.ensure(enc_table_bytes()));
    HIP_TRY(E.hdr.ensure(n * 64 + 64));
    HIP_TRY(E.size.ensure((n + 1) * 8));
    HIP_TRY(E.tmp.ensure((n + 1) * 8));
    HIP_TRY(E.cub.ensure(cub));
    EncParams P{};
    P.rec = d_records;
    P.rec_off = d_rec_off;
    P.flags = d_flags;
    P.n = n;
    P.compression = compression;
    P.scratch = E.scr.as<uint8_t>();
    P.scr_off = E.scr_off.as<uint64_t>();
    P.clen = E.clen.as<uint64_t>();
    P.gtab = E.tab.as<uint16_t>();
    P.hdr = E.hdr.as<uint8_t>();
    P.size = E.size.as<uint64_t>();
    P.tmp = E.tmp.as<uint64_t>();
    P.out = d_out;
    P.out_cap = out_cap;
    P.out_rec_off = d_out_rec_off;
    P.out_len = d_out_len;
    return hip_status(launch_encode(P, E.cub.p, E.cub.cap, stream_of(ctx, stream)));
}

extern "C" int rio_encode_file(rio_ctx* ctx, const uint8_t* records, const uint64_t* rec_off, const uint8_t* flags,
                               uint64_t n, uint32_t compression, uint8_t* out, uint64_t out_cap, uint64_t* out_rec_off,
                               uint64_t* out_len) {
    if (!ctx || !rec_off || !out_len || (n && !out_rec_off)) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::Encode& E = ctx->enc;
    const uint64_t total = rec_off[n] - rec_off[0];
    if (total && !records) return RIO_ERR_ARG;
    const uint64_t bound = rio_encode_bound(n, total, compression);
    HIP_TRY(E.rec.ensure(total + RIO_DEVICE_PAD));
    HIP_TRY(E.rec_off.ensure((n + 1) * 8));
    HIP_TRY(E.flags.ensure(n + 8));
    HIP_TRY(E.out.ensure(bound));
    HIP_TRY(E.out_off.ensure(n * 8 + 8));
    HIP_TRY(E.len.ensure(8));
    int rc = total ? h2d_staged(ctx, E.rec.p, records + rec_off[0], total) : RIO_OK;
    // offsets relative to the first record
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t i = 0; i <= n; i++) rel[i] = rec_off[i] - rec_off[0];
    if (!rc) rc = h2d_staged(ctx, E.rec_off.p, reinterpret_cast<const uint8_t*>(rel.data()), (n + 1) * 8);
    if (!rc && flags && n) rc = h2d_staged(ctx, E.flags.p, flags, n);
    if (rc) return rc;
    rc = rio_device_encode(ctx, E.rec.as<uint8_t>(), E.rec_off.as<uint64_t>(), flags ? E.flags.as<uint8_t>() : nullptr, n,
                           total, compression, E.out.as<uint8_t>(), bound, E.out_off.as<uint64_t>(), E.len.as<uint64_t>(),
                           nullptr);
    if (rc) return rc;
    uint64_t len = 0;
    rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(&len), E.len.p, 8);
    if (rc) return rc;
    *out_len = len;
    if (len > out_cap || !out) return RIO_ERR_CAPACITY;
    rc = d2h_staged(ctx, out, E.out.p, len);
    if (!rc && n) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(out_rec_off), E.out_off.p, n * 8);
    return rc;
}
