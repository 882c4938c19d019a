// rio_decode.cpp — the decode entry points of librio (include/rio.h): the device-resident calls (one file, a batch
// of files, one record, a batch of records) and the host two-phase API (rio_frame, rio_decode) the cgo binding and the reader handles use.
// Every decode runs on the device (rio_place.hip launches the pipeline); host code only moves bytes. There is no CPU decode fallback:
// a missing GPU is an error.
#include <algorithm>

#include "rio_ctx.h"

using namespace rio;

// ------------------------------------------------------------------------------------------
// device-resident single call
// ------------------------------------------------------------------------------------------
extern "C" int rio_device_decode(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint8_t* d_out,
                                 uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_rec_off, uint8_t* d_flags,
                                 uint64_t rec_cap, rio_file_info* d_info, void* stream) {
    return rio_device_decode_ex(ctx, d_file, len, RIO_COMP_UNKNOWN, d_out, out_cap, d_out_off, d_rec_off, d_flags,
                                rec_cap, d_info, stream);
}

extern "C" int rio_device_decode_ex(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint32_t compression,
                                    uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_rec_off,
                                    uint8_t* d_flags, uint64_t rec_cap, rio_file_info* d_info, void* stream) {
    if (!ctx || !d_file || !d_out_off || !d_rec_off || !d_flags || !d_info) return RIO_ERR_ARG;
    if (compression > RIO_COMP_LZW && compression != RIO_COMP_UNKNOWN) return RIO_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_file) & 15) != 0) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    FileArenas& A = ctx->fr.fa;
    FrameParams P;
    int rc = ctx_frame_params(ctx, d_file, len, P, A);
    if (rc) return rc;
    P.out = d_out;
    P.out_cap = out_cap;
    P.out_off = d_out_off;
    P.rec_off = d_rec_off;
    P.flags = d_flags;
    P.rec_cap = rec_cap;
    P.info = d_info;
    HIP_TRY(A.rec_pay.ensure((rec_cap + 1) * 8));
    P.rec_pay = A.rec_pay.as<uint64_t>();
    HIP_TRY(A.rec_desc.ensure((rec_cap + 1) * 16));
    P.rec_desc = A.rec_desc.as<uint4>();
    P.comp_hint = compression;
    hipStream_t s = stream_of(ctx, stream);
    if (int rc2 = order_before(ctx, s)) return rc2;
    hipEvent_t oe;
    if (int rc3 = order_event(ctx, oe)) return rc3;
    hipEvent_t* ev = ctx->timing.next_events();
    HIP_TRY(launch_frame(P, s, ev));
    HIP_TRY(launch_phase_b(P, s, ev, oe));
    order_mark(ctx, s);
    return RIO_OK;
}

// Batch of device-resident files (BASELINE configs[3]: the 8 files of a GPU's shard in one step):
// framing per file, then the large-record Snappy decoder once over all of them, so that files of few
// large records still fill the chip. Up to kMaxBatch files per launch group; larger batches run as
// consecutive groups on the same stream.
extern "C" int rio_device_decode_batch(rio_ctx* ctx, uint32_t n_files, const uint8_t* const* d_files,
                                       const uint64_t* lens, uint8_t* const* d_out, const uint64_t* out_cap,
                                       uint64_t* const* d_out_off, uint64_t* const* d_rec_off, uint8_t* const* d_flags,
                                       const uint64_t* rec_cap, rio_file_info* const* d_info, void* stream) {
    if (!ctx || (n_files && (!d_files || !lens || !d_out || !out_cap || !d_out_off || !d_rec_off || !d_flags ||
                             !rec_cap || !d_info)))
        return RIO_ERR_ARG;
    for (uint32_t k = 0; k < n_files; k++)
        if (!d_files[k] || (reinterpret_cast<uintptr_t>(d_files[k]) & 15) || !d_out_off[k] || !d_rec_off[k] ||
            !d_flags[k] || !d_info[k])
            return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream_of(ctx, stream);
    if (int rc = order_before(ctx, s)) return rc;
    if (n_files == 0) return RIO_OK;  // nothing enqueued: the previous call's order event still stands
    hipEvent_t oe;
    if (int rc = order_event(ctx, oe)) return rc;
    auto& batch = ctx->fr.batch;
    while (batch.size() < std::min<uint32_t>(n_files, kMaxBatch)) batch.emplace_back(new FileArenas());
    hipEvent_t* ev = ctx->timing.next_events();
    // the next call's walk hint comes from ONE file of the batch, the longest (the first of equal ones), so the choice
    // does not depend on which file's k_finish ran last
    uint32_t hint_file = 0;
    for (uint32_t k = 1; k < n_files; k++)
        if (lens[k] > lens[hint_file]) hint_file = k;
    for (uint32_t g = 0; g < n_files; g += kMaxBatch) {
        FrameBatch B{};
        B.n = std::min<uint32_t>(kMaxBatch, n_files - g);
        for (uint32_t j = 0; j < B.n; j++) {
            const uint32_t k = g + j;
            FileArenas& A = *batch[j];
            FrameParams& P = B.f[j];
            int rc = ctx_frame_params(ctx, d_files[k], lens[k], P, A);
            if (rc) return rc;
            P.out = d_out[k];
            P.out_cap = out_cap[k];
            P.out_off = d_out_off[k];
            P.rec_off = d_rec_off[k];
            P.flags = d_flags[k];
            P.rec_cap = rec_cap[k];
            P.info = d_info[k];
            HIP_TRY(A.rec_pay.ensure((rec_cap[k] + 1) * 8));
            P.rec_pay = A.rec_pay.as<uint64_t>();
            HIP_TRY(A.rec_desc.ensure((rec_cap[k] + 1) * 16));
            P.rec_desc = A.rec_desc.as<uint4>();
            if (k != hint_file) P.walk_hint = nullptr;
        }
        // stage events bracket the whole batch, on the kernels' own dispatches: [0] at the first file's walk start,
        // [1] at the last file's scan end, [2] .. [4] in launch_phase_b_batch (placement start / end, k_finish start)
        hipEvent_t* e = (ev && g == 0) ? ev : nullptr;
        hipEvent_t* last = (ev && g + kMaxBatch >= n_files) ? ev : nullptr;
        for (uint32_t j = 0; j < B.n; j++)
            HIP_TRY(launch_frame_ev(B.f[j], s, (e && j == 0) ? e[0] : nullptr, nullptr,
                                    (last && j + 1 == B.n) ? last[1] : nullptr));
        HIP_TRY(launch_phase_b_batch(B, s, last, g + kMaxBatch >= n_files ? oe : nullptr));
    }
    order_mark(ctx, s);
    return RIO_OK;
}

// single-record decode (ReadNextAt) on a device-resident file
extern "C" int rio_device_read_at(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t offset,
                                  uint8_t* d_out, uint64_t out_cap, uint64_t* len_out, int* nil_out,
                                  uint64_t* detail0, uint64_t* detail1) {
    if (!ctx || !d_file) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ReadAtResult r{};
    DevBuf& res = ctx->host.readat_res;
    HIP_TRY(res.ensure(sizeof(ReadAtResult)));
    HIP_TRY(launch_read_at(d_file, len, offset, d_out, out_cap, res.as<ReadAtResult>(), ctx->stream));
    HIP_TRY(hipMemcpyAsync(&r, res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (len_out) *len_out = r.len;
    if (nil_out) *nil_out = r.nil;
    if (detail0) *detail0 = r.det0;
    if (detail1) *detail1 = r.det1;
    return r.status;
}

// a batch of ReadNextAt queries on a device-resident file: the plan / copy pair (k_readat_locate, k_readat_copy:
// rio_seek.hip; k_readat_snappy: rio_snappy.hip). Stream-ordered. No host synchronisation but one: the context's scan
// arenas only grow, and a DevBuf that grows frees its old allocation with hipFree, which waits for the device. The arenas
// are the context's, so one context serves one stream at a time for these calls (rio.h)
static int read_at_batch_args(const rio_ctx* ctx, const uint8_t* d_file, uint64_t n, const void* a, const void* b,
                              const void* c) {
    if (!ctx || !d_file || (reinterpret_cast<uintptr_t>(d_file) & 15) != 0) return RIO_ERR_ARG;
    if (n && (!a || !b || !c)) return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    return RIO_OK;
}

extern "C" int rio_device_read_at_plan(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, const uint64_t* d_offsets,
                                       uint64_t n, rio_read_at_hit* d_hits, uint64_t* d_out_off, void* stream) {
    if (int rc = read_at_batch_args(ctx, d_file, n, d_offsets, d_hits, d_out_off)) return rc;
    if (n == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::ReadAtBatch& B = ctx->rab;
    HIP_TRY(B.tmp.ensure((n + 1) * 8));
    HIP_TRY(B.cub.ensure(std::max<size_t>(scan_cub_bytes(n), 256)));
    ReadAtParams P{};
    P.file = d_file;
    P.len = len;
    P.offsets = d_offsets;
    P.n = n;
    P.hits = reinterpret_cast<ReadAtResult*>(d_hits);
    P.tmp = B.tmp.as<uint64_t>();
    P.out_off = d_out_off;
    return hip_status(launch_read_at_plan(P, B.cub.p, B.cub.cap, stream_of(ctx, stream)));
}

extern "C" int rio_device_read_at_copy(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t n,
                                       rio_read_at_hit* d_hits, const uint64_t* d_out_off, uint8_t* d_out,
                                       uint64_t out_cap, void* stream) {
    if (int rc = read_at_batch_args(ctx, d_file, n, d_hits, d_out_off, d_out)) return rc;
    if (n == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->fr.sink.ensure(kSinkBytes));
    ReadAtParams P{};
    P.file = d_file;
    P.len = len;
    P.n = n;
    P.hits = reinterpret_cast<ReadAtResult*>(d_hits);
    P.out_off = const_cast<uint64_t*>(d_out_off);
    P.out = d_out;
    P.out_cap = out_cap;
    P.sink = ctx->fr.sink.as<uint8_t>();
    hipStream_t s = stream_of(ctx, stream);
    HIP_TRY(launch_read_at_copy(P, s));
    return hip_status(launch_read_at_snappy(P, s));
}

// ------------------------------------------------------------------------------------------
// host two-phase API (cgo)
// ------------------------------------------------------------------------------------------
// the host API's output arenas for n records of nb decoded bytes, and the file's descriptors
static int ensure_outputs(rio_ctx* ctx, uint64_t n, uint64_t nb) {
    rio_ctx::HostApi& H = ctx->host;
    HIP_TRY(H.out.ensure(nb + 16));
    HIP_TRY(H.out_off.ensure((n + 1) * 8));
    HIP_TRY(H.rec_off.ensure(n * 8 + 8));
    HIP_TRY(H.flags.ensure(n + 8));
    HIP_TRY(ctx->fr.fa.rec_pay.ensure((n + 1) * 8));
    HIP_TRY(ctx->fr.fa.rec_desc.ensure((n + 1) * 16));
    return RIO_OK;
}

// phase B's parameters after phase A's P: decode into the host API's arenas
static FrameParams decode_params(rio_ctx* ctx, const FrameParams& P, uint32_t compression, uint64_t n, uint64_t nb) {
    rio_ctx::HostApi& H = ctx->host;
    FrameParams D = P;
    D.zero_done = 1;  // phase A ran k_zero (rio_frame's status is final)
    D.comp_hint = compression;  // from the file header rio_frame read
    D.out = H.out.as<uint8_t>();
    D.out_cap = nb;
    D.out_off = H.out_off.as<uint64_t>();
    D.rec_off = H.rec_off.as<uint64_t>();
    D.flags = H.flags.as<uint8_t>();
    D.rec_cap = n;
    D.rec_pay = ctx->fr.fa.rec_pay.as<uint64_t>();
    D.rec_desc = ctx->fr.fa.rec_desc.as<uint4>();
    return D;
}

// the decoded records of D (n records, nb bytes) to the caller's host arrays
static int fetch_outputs(rio_ctx* ctx, const FrameParams& D, uint64_t n, uint64_t nb, uint8_t* out, uint64_t* out_off,
                         uint64_t* rec_off, uint8_t* flags) {
    int rc;
    if (nb && (rc = d2h_staged(ctx, out, D.out, nb))) return rc;
    if (out_off && (rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(out_off), D.out_off, (n + 1) * 8))) return rc;
    if (n) {
        if ((rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(rec_off), D.rec_off, n * 8))) return rc;
        if ((rc = d2h_staged(ctx, flags, D.flags, n))) return rc;
    }
    return RIO_OK;
}

// `prefix` (prefix_len bytes, host) then `file` (len - prefix_len bytes): a window of a larger file
// behind its file header (rio::frame_direct)
static int frame_common(rio_ctx* ctx, uint64_t len, rio_file_info* info, const uint8_t* file, rio::FillFn fill,
                        void* user, const uint8_t* prefix = nullptr, uint64_t prefix_len = 0) {
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::HostApi& H = ctx->host;
    // the host API shares the ctx arenas with the device API: wait for a device-API call still
    // running on another stream, and make the next device-API call wait for this one
    if (int rc = order_before(ctx, ctx->stream)) return rc;
    H.framed = false;
    HIP_TRY(H.file.ensure(len + RIO_DEVICE_PAD));
    if (prefix_len) HIP_TRY(hipMemcpyAsync(H.file.p, prefix, prefix_len, hipMemcpyHostToDevice, ctx->stream));
    int rc = fill ? h2d_fill(ctx, H.file.p, len, fill, user)
                  : h2d_staged(ctx, H.file.as<uint8_t>() + prefix_len, file, len - prefix_len);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(H.file.as<uint8_t>() + len, 0, RIO_DEVICE_PAD, ctx->stream));
    FrameParams P;
    rc = ctx_frame_params(ctx, H.file.as<uint8_t>(), len, P, ctx->fr.fa);
    if (rc) return rc;
    HIP_TRY(launch_phase_a(P, ctx->stream, ctx->timing.next_events()));
    HIP_TRY(hipMemcpyAsync(&H.frame_info, P.info, sizeof(rio_file_info), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    H.predecoded = false;
    const rio_file_info& fi = H.frame_info;
    const bool expand = fi.compression == RIO_COMP_GZIP || fi.compression == RIO_COMP_LZW;
    if (expand && !nothing_framed(fi.status)) {
        // gzip / lzw: decode now. The framing sizes a gzip record from its last member's ISIZE, an lzw
        // record from its header's u; a record of several gzip members (Go's multistream reader) is
        // larger, an lzw record under a header that lies differs, which only the decode finds out, and
        // the caller allocates from the sizes returned here. A decode that needs more room than the
        // framing's sizes reports RIO_ERR_CAPACITY with the sizes it needs: frame and decode again
        // into arenas of that size (the whole pipeline: framing resets the device state).
        uint64_t n = fi.n_records, nb = fi.total_out_bytes;
        rio_file_info fin{};
        for (int attempt = 0; attempt < 3; attempt++) {
            if ((rc = ensure_outputs(ctx, n, nb))) return rc;
            if (attempt) HIP_TRY(launch_phase_a(P, ctx->stream, nullptr));
            const FrameParams D = decode_params(ctx, P, fi.compression, n, nb);
            HIP_TRY(launch_phase_b(D, ctx->stream, attempt ? nullptr : ctx->timing.same_events()));
            HIP_TRY(hipMemcpyAsync(&fin, D.info, sizeof fin, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            P = D;
            if (fin.status != RIO_ERR_CAPACITY) break;
            n = fin.n_records;
            nb = fin.total_out_bytes;
        }
        if (fin.status == RIO_ERR_CAPACITY) return RIO_ERR_CAPACITY;
        H.frame_info = fin;
        H.predecoded = true;
    }
    *info = H.frame_info;
    H.last = P;
    H.framed = true;
    return order_after(ctx, ctx->stream);
}

extern "C" int rio_frame(rio_ctx* ctx, const uint8_t* file, uint64_t len, rio_file_info* info) {
    if (!ctx || (!file && len) || !info) return RIO_ERR_ARG;
    return frame_common(ctx, len, info, file, nullptr, nullptr);
}

int rio::frame_fill(rio_ctx* ctx, uint64_t len, FillFn fill, void* user, rio_file_info* info) {
    if (!ctx || !fill || !info) return RIO_ERR_ARG;
    return frame_common(ctx, len, info, nullptr, fill, user);
}
int rio::frame_direct(rio_ctx* ctx, const uint8_t* prefix, uint64_t prefix_len, const uint8_t* src, uint64_t n,
                      rio_file_info* info) {
    if (!ctx || !info || (n && !src) || (prefix_len && !prefix)) return RIO_ERR_ARG;
    return frame_common(ctx, prefix_len + n, info, src, nullptr, nullptr, prefix, prefix_len);
}

extern "C" int rio_decode(rio_ctx* ctx, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* rec_off,
                          uint8_t* flags, uint64_t rec_cap, rio_file_info* info) {
    if (!ctx || !info) return RIO_ERR_ARG;
    rio_ctx::HostApi& H = ctx->host;
    if (!H.framed) return RIO_ERR_STATE;
    HIP_TRY(hipSetDevice(ctx->device));
    const rio_file_info fi = H.frame_info;
    if (nothing_framed(fi.status)) {
        *info = fi;
        return RIO_OK;
    }
    const uint64_t n = fi.n_records, nb = fi.total_out_bytes;
    if (rec_cap < n || out_cap < nb || (n && (!out_off || !rec_off || !flags)) || (nb && !out)) return RIO_ERR_CAPACITY;
    if (int rc = order_before(ctx, ctx->stream)) return rc;
    if (H.predecoded) {  // gzip: rio_frame decoded the file (its sizes are the decoded ones)
        if (int rc = fetch_outputs(ctx, H.last, n, nb, out, out_off, rec_off, flags)) return rc;
        *info = fi;
        return order_after(ctx, ctx->stream);
    }
    if (int rc = ensure_outputs(ctx, n, nb)) return rc;
    const FrameParams P = decode_params(ctx, H.last, fi.compression, n, nb);
    HIP_TRY(launch_phase_b(P, ctx->stream, ctx->timing.same_events()));
    rio_file_info fin{};
    HIP_TRY(hipMemcpyAsync(&fin, P.info, sizeof fin, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (int rc = fetch_outputs(ctx, P, fin.n_records, fin.total_out_bytes, out, out_off, rec_off, flags)) return rc;
    *info = fin;
    return order_after(ctx, ctx->stream);
}
