// rio_place.hip — placement, the record copy and the last step of the recordio v3/v4 decode path on CDNA4 (gfx950),
// and the launch sequence of the whole pipeline.
//
// Pipeline for one file already in HBM: six launches for a Snappy file when the
// host passes the codec (rio_device_decode_ex), follow-up steps run by the last block to arrive.
//   k_walk / k_walk_lane   (rio_walk.hip) a wave per 32 KiB chunk, or a lane per small chunk: speculative entry and
//                   the records walked from it to per-chunk scratch; also reads the file header
//                   (readFileHeaderFromBuffer, common_reader.go:22-44) and resets ScanState.
//   k_scan_blocks   (rio_chunk_scan.hip) inclusive scan of key-point chunk summaries, the repair walk where an
//                   entry does not chain, record/byte prefix sums, terminal status.
//   k_place         prologue: arena capacity, zero-tail check behind a magic mismatch
//                   (file_reader.go:76-91); scratch -> rec_off / out_off / flags at their global index.
//   k_copy_records  uncompressed payloads and single-literal Snappy records (16-lane copies).
//   k_snappy_pipe   golang/snappy v1.0.0 block decode (rio_snappy.hip); k_gzip_* (rio_gzip.hip); k_lzw_* (rio_lzw.hip).
//   k_finish        re-check of records handed over by decoder lanes; last block: rio_file_info.
// Host-API phase A (rio_frame) adds k_zero + k_finalize after the scan. The seek map and the single-record
// k_read_at / k_seek_next that serve the ReadAtI handle are in rio_seek.hip.
// Byte/integer work only: no MFMA. All offsets 64-bit.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_frame.h"
#include "rio_launch.h"
#include "rio_wave.h"

namespace rio {

// Header length of a snappy stream that is one literal element producing exactly `len` bytes with
// nothing after it, or 0 (an empty stream for an empty record counts as such, header length 0 is
// then harmless). Tag 00: literal, length - 1 = tag >> 2, or 60..63 => 1..4 little-endian bytes.
__device__ __forceinline__ uint32_t snappy_literal_hdr(const uint8_t* p, uint64_t slen, uint64_t len) {
    if (slen == 0) return len == 0 ? 1u : 0u;
    // one literal = 1..5 header bytes + exactly len data bytes: decided from the sizes alone for
    // every compressible record, so only candidates cost a load
    if (slen <= len || slen > len + 5) return 0;
    const uint32_t tag = p[0];
    if (tag & 3u) return 0;
    const uint32_t x = tag >> 2;
    uint64_t L;
    uint32_t h;
    if (x < 60) {
        L = (uint64_t)x + 1;
        h = 1;
    } else {
        const uint32_t nb = x - 59;
        if (slen < 1 + nb) return 0;
        uint64_t v = 0;
        for (uint32_t b = 0; b < nb; b++) v |= (uint64_t)p[1 + b] << (8 * b);
        L = v + 1;
        h = 1 + nb;
    }
    return (L == len && h + L == slen) ? h : 0u;
}
__device__ __forceinline__ bool snappy_single_literal(const uint8_t* p, uint64_t slen, uint64_t len) {
    return snappy_literal_hdr(p, slen, len) != 0;
}

// A chunk's records, placed: file records [base_idx, base_idx + owned) are chunk c's scratch slots
// [0, owned); rec_off / rec_pay / out_off / flags / rec_desc at their global index, 64 records per wave
// step, out_off by a wave prefix sum (coalesced stores instead of one thread's serial record loop).
// `snappy`: look for a record that is not one literal element of its whole length (the probe stops at
// the first). What the chunk found goes back to the caller, which merges it into ScanState.
struct PlaceFlags {
    uint64_t first_bad;  // first record flagged at framing (kNone: none)
    uint64_t n_bad;
    bool mixed;          // a Snappy record that is not one literal (or the probe was off)
    bool huge;           // a stream or record past 32-bit sizes
};

template <uint32_t G>
__device__ PlaceFlags place_chunk(const FrameParams& P, uint64_t c, uint64_t base_idx, uint64_t base_bytes,
                                  uint64_t owned, bool snappy, bool pay_all, uint32_t lane) {
    PlaceFlags fl{kNone, 0, false, false};
    const uint64_t cs = chunk_start(P, c);
    const WalkSlot* sc = P.scratch + c * P.slots;
    bool mixed = false, huge = false;
    uint64_t carry = base_bytes;
    // the slots of the next 64 records loaded before this step's stores: on CDNA vmcnt retires loads
    // and stores in issue order, so a load issued after the stores would wait for them
    WalkSlot s_n{0, 0};
    if (lane < owned) s_n = slot_load(sc + lane);
    for (uint64_t k0 = 0; k0 < owned; k0 += G) {
        const uint64_t k = k0 + lane;
        const bool v = k < owned;
        const uint64_t l = s_n.len, ro = cs + slot_rel(s_n.pos), len = v ? l & kLenMask : 0;
        uint64_t pay = slot_pay(s_n.pos);
        const bool esc = v && (s_n.pos & kSlotEsc);
        if (k + G < owned) s_n = slot_load(sc + k + G);
        if (esc) {
            // an escaped slot (WalkSlot): the stream ends where the chain's next record starts, which is the next
            // slot's record or, behind the chunk's last record, where the walk left the chunk (ChunkSum::exit)
            const uint64_t nx = k + 1 < owned ? cs + slot_rel(sc[k + 1].pos) : P.chunks[c].exit;
            pay |= (nx - ro - pay) << 8;
        }
        uint64_t wsum;
        const uint64_t excl = G == 64 ? wave_excl_scan64(len, lane, wsum) : group16_excl_scan64(len, lane, wsum);
        bool bad = false;
        if (v) {
            const uint64_t i = base_idx + k;
            const uint64_t start = ro + (pay & 0xFF), slen = pay >> 8;
            // rec_pay only where a consumer needs it (rec_stream): the stream position and length of a
            // snappy / uncompressed record travel in rec_desc
            const bool wide = slen >= kDescWide || len >= kDescWide;
            P.rec_off[i] = ro;
            if (pay_all || wide) P.rec_pay[i] = pay;
            P.out_off[i] = carry + excl;
            const uint8_t fg = ((l & kNilBit) ? RIO_FLAG_NIL : 0) | ((l & kBadBit) ? RIO_FLAG_CORRUPT : 0) |
                               ((l & kEofBit) ? RIO_FLAG_EOF : 0);
            P.flags[i] = fg;
            bad = (fg & (RIO_FLAG_CORRUPT | RIO_FLAG_EOF)) != 0;  // failed at framing (stream length 0)
            P.rec_desc[i] = make_uint4((uint32_t)start, (uint32_t)(start >> 32), wide ? kDescWide : (uint32_t)slen,
                                       wide ? kDescWide : (uint32_t)len);
            huge = huge || wide;  // (also a size of exactly 2^32 - 1: rec_desc holds the sentinel)
            // a snappy stream that is exactly one literal element of the record's whole length
            // (what golang/snappy emits for incompressible input) decodes as a copy
            if (snappy && fg == 0) mixed |= !snappy_single_literal(P.file + start, slen, len);
        }
        const uint64_t bm = group_ballot<G>(bad);
        if (bm) {
            fl.n_bad += (uint64_t)__popcll(bm);
            if (fl.first_bad == kNone) fl.first_bad = base_idx + k0 + (uint64_t)__builtin_ctzll(bm);
        }
        carry += wsum;
        snappy = snappy && !group_ballot<G>(mixed);
        mixed = mixed || !snappy;  // keep the group's verdict
    }
    fl.mixed = group_ballot<G>(mixed) != 0;
    fl.huge = group_ballot<G>(huge) != 0;
    return fl;
}

// a chunk's flags into the file's state (one lane)
__device__ __forceinline__ void merge_place_flags(const FrameParams& P, const PlaceFlags& f) {
    ScanState* st = P.state;
    if (f.first_bad != kNone) atomicMin((unsigned long long*)&st->first_bad, (unsigned long long)f.first_bad);
    if (f.n_bad) atomicAdd((unsigned long long*)&st->n_bad, (unsigned long long)f.n_bad);
    if (f.huge) atomicOr(&st->huge_streams, 1u);
    // every writer stores the same 1: a plain store, not an atomic (17 k same-address atomics from
    // the chunk waves of a 1 M-record file serialized at L2 and cost 0.35 ms)
    if (f.mixed && st->compression == RIO_COMP_SNAPPY) st->any_mixed = 1u;
}

// Placement: one wave per chunk (place_chunk). Its prologue also does what used to be two launches:
// the capacity check + sentinel out_off[n] (block 0) and, on the device-resident path, the zero-tail
// test of a magic mismatch (grid-stride).
// G lanes per chunk: 64 (a wave) for the wave walk's 32 KiB chunks, 16 for the lane walk's small ones (2..21
// records of 768 B .. 8 KiB: a wave per chunk left most lanes idle, C2-ref-random place 0.058 -> 0.080 ms)
template <uint32_t G>
__global__ void __launch_bounds__(256) k_place(FrameParams P) {
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    ScanState* st = P.state;
    const uint32_t pf = code_pf(blockIdx.x < kPfBlocks ? kPfPlace : 0);
    if (st->hdr_status != RIO_OK) return;
    if (P.redo && (!st->gz_redo || st->compression != P.redo)) return;  // another codec's redo round
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (st->n_records > P.rec_cap || st->total_bytes > P.out_cap)
            st->capacity_fail = 1;
        else
            P.out_off[st->n_records] = st->total_bytes;
    }
    if (!P.zero_done && st->zero_from != kNone) {
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        uint32_t nz = 0;
        for (uint64_t q = st->zero_from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < P.len; q += stride)
            nz |= P.file[q];
        if (__any(nz != 0) && lane == 0) atomicOr(&st->zero_nonzero, 1u);
    }
    if (c >= P.n_chunks) return;  // wave-uniform
    ChunkPlace pl;
    if (st->slow) {
        pl = P.place[c];
    } else {
        const uint64_t b = c / kScanBlock;
        const RunSum B = P.block_excl[b];
        const RunSum E = P.chunk_excl[c];
        // chain position entering block b (block 0 is entered at 8 = its forced key). A block
        // owns records only if the chain enters it exactly at its key; otherwise it was passed
        // through (a record spans it) or the chain terminated before it.
        const uint64_t xb = (b == 0) ? (uint64_t)RIO_FILE_HEADER_BYTES : B.out;
        const bool entered = (b == 0) || (!B.term && !B.broken && xb == P.block_runs[b].key);
        pl.owned = 0;
        pl.base_idx = B.cnt + E.cnt;
        pl.base_bytes = B.bytes + E.bytes;
        if (entered && !E.term && !E.broken) {
            const uint64_t y = (E.key == kNone) ? xb : E.out;
            const ChunkSum s = P.chunks[c];
            if (s.entry != kNone && y == s.entry) pl.owned = s.count;
        }
        if (lane == 0) P.place[c] = pl;
    }
    if (pl.owned == 0) return;
    if (pl.base_idx + pl.owned > P.rec_cap || st->n_records > P.rec_cap) return;
    // once any wave has found a mixed record the file takes k_snappy_pipe: later waves skip the probe
    const bool snappy = st->compression == RIO_COMP_SNAPPY && !*(volatile const uint32_t*)&st->any_mixed;
    const bool pay_all = st->compression == RIO_COMP_GZIP || st->compression == RIO_COMP_LZW;
    const PlaceFlags f = place_chunk<G>(P, c, pl.base_idx, pl.base_bytes, pl.owned, snappy, pay_all, lane);
    if (lane == 0) merge_place_flags(P, f);
    code_pf_done(pf);
}

__global__ void __launch_bounds__(256) k_zero(FrameParams P) {
    ScanState* st = P.state;
    const uint64_t from = st->zero_from;
    if (from == kNone || st->hdr_status != RIO_OK) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t nz = 0;
    for (uint64_t q = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < P.len; q += stride)
        nz |= P.file[q];
    if (nz) atomicOr(&st->zero_nonzero, 1u);
}

// ------------------------------------------------------------------------------------------
// Decode
// ------------------------------------------------------------------------------------------
// dst[d, d+len) = src[0, len), 16 bytes at a time; whole 16-byte stores may overrun the element
// (later elements overwrite those bytes) but never the record end `dlen`.
__device__ __forceinline__ void copy_fwd(uint8_t* dst, uint64_t d, const uint8_t* src, uint64_t len, uint64_t dlen) {
    for (uint64_t k = 0; k < len; k += 16) {
        const uint4 v = ldu16(src + k);
        if (d + k + 16 <= dlen)
            stu16(dst + d + k, v);
        else
            st_partial(dst + d + k, v, (uint32_t)(dlen - d - k));
    }
}

// Uncompressed files, and Snappy files whose every record is one literal (incompressible values:
// the reference benchmark's random records; k_snappy_pipe exits at once for those): 16-lane groups,
// one record per group; each lane moves 16 bytes per step (unaligned load and store; the record's
// last piece is stored exactly).
// kG lanes per record (16, or 4 for files of small records: their 16-lane groups left 12 lanes idle and took a
// dependent round trip per 50-byte record, C5's index copy 0.12 ms for 61 MB); each group's next record's sizes
// are loaded while the current one is copied, and a record moves in rounds of 64 kG bytes (four 16-byte loads per
// lane in flight, then the four stores): the copy was a chain of dependent round trips (sizes, literal header
// byte, then 256 bytes at a time)
template <uint32_t kG>
__device__ __forceinline__ void copy_groups(const FrameParams& P, uint64_t n, bool none) {
    const uint32_t lane = threadIdx.x & (kG - 1);
    const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kG;
    const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / kG;
    auto meta = [&](uint64_t i, uint64_t& o0, uint64_t& len, const uint8_t*& src) __attribute__((always_inline)) {
        o0 = P.out_off[i];
        len = P.out_off[i + 1] - o0;
        uint64_t start, slen;
        rec_stream(P, i, start, slen);
        // a Snappy record here is one literal of its whole length (k_place checked every record with
        // bytes): its header is the slen - len bytes in front of them, no byte to read
        src = P.file + start + (none ? 0 : slen - len);
    };
    uint64_t o0 = 0, len = 0;
    const uint8_t* src = P.file;
    if (grp < n) meta(grp, o0, len, src);
    for (uint64_t i = grp; i < n; i += ngrp) {
        uint64_t no0 = 0, nlen = 0;
        const uint8_t* nsrc = P.file;
        if (i + ngrp < n) meta(i + ngrp, no0, nlen, nsrc);
        uint8_t* dst = P.out + o0;
        for (uint64_t k0 = 0; k0 < len; k0 += 64 * kG) {
            uint4 v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t k = k0 + 16 * kG * j + 16 * lane;
                v[j] = k < len ? ldu16_nt(src + k) : zero4();
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t k = k0 + 16 * kG * j + 16 * lane;
                if (k + 16 <= len) {
                    stu16_nt(dst + k, v[j]);
                } else if (k < len) {
                    st_partial(dst + k, v[j], (uint32_t)(len - k));
                }
            }
        }
        o0 = no0;
        len = nlen;
        src = nsrc;
    }
}

// k_copy_records (round 5): the next record's sizes prefetched and 1 KiB in flight per 16-lane group, non-temporal loads
// and stores (C2-ref-random copy 0.423 -> 0.370 ms, 5.8 TB/s; C1 +7 %, C5 +4 % against plain ones and the round-4 loop:
// profiles/r5/r5aa_copy_ab.txt)
// k_copy_records' grid (4096 x 256: C1's 100 k records over twice the groups, copy 0.067 -> 0.057 ms; C2-ref-random
// -2 %; 1024: C1 +45 %; two records in flight per group: +10 %, r5ab)
constexpr unsigned kCopyGrid = 4096;
// files whose records average fewer bytes than this copy with 4 lanes per record instead of 16
constexpr uint64_t kCopySmall = 128;
__global__ void __launch_bounds__(256) k_copy_records(FrameParams P) {
    const ScanState* st = P.state;
    const uint32_t pf = code_pf(blockIdx.x < kPfBlocks ? kPfCopy : 0);
    if (st->hdr_status != RIO_OK || st->capacity_fail) return;
    const bool none = st->compression == RIO_COMP_NONE;
    if (!none && !(st->compression == RIO_COMP_SNAPPY && !st->any_mixed)) return;
    const uint64_t n = st->n_records;
    // wave-uniform: the file's mean record size picks the group width
    if (st->total_bytes < kCopySmall * n)
        copy_groups<4>(P, n, none);
    else
        copy_groups<16>(P, n, none);
    code_pf_done(pf);
}

__device__ void finalize_info(const FrameParams& P) {
    // the file's mean bytes per record, for the context's choice of walk on its next decode (ctx_frame_params)
    if (P.walk_hint && P.state->n_records && P.len > RIO_FILE_HEADER_BYTES)
        *reinterpret_cast<volatile uint64_t*>(P.walk_hint) = (P.len - RIO_FILE_HEADER_BYTES) / P.state->n_records;
    ScanState* st = P.state;
    rio_file_info info;
    info.version = st->version;
    info.compression = st->compression;
    info.reserved0 = 0;
    info.n_chunks = P.n_chunks;
    info.n_repairs = st->n_repairs;
    info.detail0 = 0;
    info.detail1 = 0;
    info.first_bad = kNone;
    info.n_bad = 0;
    if (st->hdr_status != RIO_OK) {
        info.n_records = 0;
        info.total_out_bytes = 0;
        info.status = st->hdr_status;
        info.status_offset = 0;
        info.detail0 = st->det0;
        *P.info = info;
        return;
    }
    info.n_records = st->n_records;
    info.total_out_bytes = st->total_bytes;
    info.status = st->status;
    info.status_offset = st->status_offset;
    info.detail0 = st->det0;
    info.detail1 = st->det1;
    if (st->status == RIO_ERR_MAGIC && st->zero_from != kNone && !st->zero_nonzero) {
        info.status = RIO_EOF_ZERO_TAIL;
        info.detail0 = 0;
    }
    info.first_bad = kNone;
    info.n_bad = 0;
    if (st->capacity_fail) {
        info.status = RIO_ERR_CAPACITY;
    } else {
        // a record the device path hands back ends the sequence there (the adapter re-reads the file)
        const uint64_t u = st->unsupported_rec;
        if (u != kNone && u < st->n_records) {
            info.n_records = u;
            info.total_out_bytes = P.out_off[u];
            info.status = RIO_ERR_UNSUPPORTED;
            info.status_offset = P.rec_off[u];
            info.detail0 = info.detail1 = 0;
        }
        if (st->first_bad < info.n_records) {
            info.first_bad = st->first_bad;
            info.n_bad = st->n_bad;  // (records past a hand-back point never reach this kernel's view)
        }
    }
    if (P.comp_hint != RIO_COMP_UNKNOWN && st->hdr_status == RIO_OK && st->compression != P.comp_hint) {
        info.status = RIO_ERR_ARG;  // the caller's hint launched another codec's kernels: nothing decoded
        info.n_records = 0;
        info.total_out_bytes = 0;
    }
    *P.info = info;
}

// The framing result (host API phase A: the sizes the caller allocates for)
__global__ void k_finalize(FrameParams P) {
    if (threadIdx.x == 0 && blockIdx.x == 0) finalize_info(P);
}

// Last decode step: records of Snappy lanes that met a corrupt record are decoded again one thread
// each (k_snappy_pipe lists the lanes; every record when more than kFailLanes did) in place (a record
// that decoded is rewritten with the same bytes) and flagged where golang/snappy's Decode returns
// ErrCorrupt; then the last block to finish publishes the result (k_finalize's work). One launch.
__device__ __forceinline__ void finish_file(const FrameParams& P) {
    __shared__ uint32_t last;
    ScanState* st = P.state;
    const uint32_t pf = code_pf(kPfFinish);
    if (st->hdr_status == RIO_OK && !st->capacity_fail && st->compression == RIO_COMP_SNAPPY && st->n_fail_lanes) {
        auto verify = [&](uint64_t i) {
            if (P.flags[i] & (RIO_FLAG_NIL | RIO_FLAG_CORRUPT | RIO_FLAG_EOF)) return;
            const uint64_t o0 = P.out_off[i], o1 = P.out_off[i + 1];
            uint64_t start, slen;
            rec_stream(P, i, start, slen);
            if (!snappy_decode_thread(P.file + start, slen, P.out + o0, o1 - o0))
                mark_bad(P, i);
        };
        if (st->n_fail_lanes > kFailLanes) {  // the list overflowed: every record
            const uint64_t n = st->n_records, stride = (uint64_t)gridDim.x * blockDim.x;
            for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) verify(i);
        } else {
            for (uint64_t l = blockIdx.x; l < st->n_fail_lanes; l += gridDim.x)
                for (uint64_t i = P.fail_lanes[2 * l] + threadIdx.x; i < P.fail_lanes[2 * l + 1]; i += blockDim.x)
                    verify(i);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(&st->finish_ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        __threadfence();
        finalize_info(P);
    }
    code_pf_done(pf);
}

__global__ void __launch_bounds__(256) k_finish(FrameParams P) { finish_file(P); }
// the files of a batch in one launch: blockIdx.y is the file (each file's 64 blocks take its own ticket)
__global__ void __launch_bounds__(256) k_finish_batch(FrameBatch B) { finish_file(B.f[blockIdx.y]); }

// ------------------------------------------------------------------------------------------
// Host-side launchers of the decode pipeline (declared in rio_launch.h, called by the host runtime)
// ------------------------------------------------------------------------------------------
// Framing: the walk (file header, state reset, chunk walk: rio_walk.hip), k_scan_blocks (both scan levels:
// rio_chunk_scan.hip). walk_start / walk_stop / scan_stop: the stage events (any may be null).
hipError_t launch_frame_ev(const FrameParams& P, hipStream_t s, hipEvent_t walk_start, hipEvent_t walk_stop,
                           hipEvent_t scan_stop) {
    launch_walk(P, s, walk_start, walk_stop);
    launch_chunk_scan(P, s, scan_stop);
    return hipGetLastError();
}
hipError_t launch_frame(const FrameParams& P, hipStream_t s, hipEvent_t* ev) {
    return ev ? launch_frame_ev(P, s, ev[0], ev[1], ev[2]) : launch_frame_ev(P, s, nullptr, nullptr, nullptr);
}

// k_place: 16 lanes per chunk for the lane walk's chunks, a wave for the wave walk's
static void launch_place(const FrameParams& P, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
    if (P.walk_lane)
        launch_ev(k_place<16>, dim3(blocks_for(P.n_chunks, 16)), dim3(256), s, start, stop, P);
    else
        launch_ev(k_place<64>, dim3(blocks_for(P.n_chunks, 4)), dim3(256), s, start, stop, P);
}

// Host API phase A: framing, then the zero-tail test and the sizes (k_finalize) for the caller.
hipError_t launch_phase_a(const FrameParams& P, hipStream_t s, hipEvent_t* ev) {
    launch_frame(P, s, ev);
    hipLaunchKernelGGL(k_zero, dim3(256), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, s, P);
    return hipGetLastError();
}

// gzip redo round: records holding several members (Go's multistream reader) are sized by
// k_gz_resize; then the scan, placement and gzip decoders run again with the corrected sizes. Every
// kernel of the round exits at once unless a record needed it.
static void launch_gzip_redo(const FrameParams& P0, hipStream_t s) {
    FrameParams P = P0;
    P.redo = RIO_COMP_GZIP;
    launch_gzip_resize(P, s);
    launch_chunk_scan(P, s, nullptr);
    launch_place(P, s);
    launch_gzip_decode(P, s);
}

// the same round for lzw records whose decoded size is not the header's u
static void launch_lzw_redo(const FrameParams& P0, hipStream_t s) {
    FrameParams P = P0;
    P.redo = RIO_COMP_LZW;
    launch_lzw_resize(P, s);
    launch_chunk_scan(P, s, nullptr);
    launch_place(P, s);
    launch_lzw_decode(P, s);
}

// the decoders of one file: by the compression hint, or all of them (each exits unless the file is
// its own)
static void launch_decoders(const FrameParams& P, hipStream_t s, bool snappy_main) {
    const uint32_t c = P.comp_hint;
    const bool any = c == RIO_COMP_UNKNOWN;
    if (any || c == RIO_COMP_NONE || c == RIO_COMP_SNAPPY)
        hipLaunchKernelGGL(k_copy_records, dim3(kCopyGrid), dim3(256), 0, s, P);
    if ((any || c == RIO_COMP_SNAPPY) && snappy_main) launch_snappy_decode(P, s, true);
    if (any || c == RIO_COMP_GZIP) {
        launch_gzip_decode(P, s);
        launch_gzip_redo(P, s);
    }
    if (any || c == RIO_COMP_LZW) {
        launch_lzw_decode(P, s);
        launch_lzw_redo(P, s);
    }
}

// Decode: placement (+ capacity check, zero tail), the decoders, k_finish (verify + result).
// stage events: [3] at the placement's end, [4] at k_finish's start, so the decode stage is the decoders' span;
// `done` (the context's order event) completes with k_finish
hipError_t launch_phase_b(const FrameParams& P, hipStream_t s, hipEvent_t* ev, hipEvent_t done) {
    launch_place(P, s, nullptr, ev ? ev[3] : nullptr);
    launch_decoders(P, s, true);
    launch_ev(k_finish, dim3(64), dim3(256), s, ev ? ev[4] : nullptr, done, P);
    return hipGetLastError();
}

// rio_device_decode_batch: phase B of every file of the batch; the Snappy decoders run once over all
// of them (k_snappy_pipe_batch / k_snappy_coop_batch), the other decode kernels per file
// stage events: [2] at the first placement's start (the framing of every file ends at [1]), [3] at the last
// placement's end, [4] at k_finish_batch's start
hipError_t launch_phase_b_batch(const FrameBatch& B, hipStream_t s, hipEvent_t* ev, hipEvent_t done) {
    for (uint32_t f = 0; f < B.n; f++)
        launch_place(B.f[f], s, (ev && f == 0) ? ev[2] : nullptr, (ev && f + 1 == B.n) ? ev[3] : nullptr);
    launch_snappy_batch(B, s);
    for (uint32_t f = 0; f < B.n; f++) launch_decoders(B.f[f], s, false);
    launch_ev(k_finish_batch, dim3(64, B.n), dim3(256), s, ev ? ev[4] : nullptr, done, B);
    return hipGetLastError();
}
}  // namespace rio
