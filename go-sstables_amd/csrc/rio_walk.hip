// rio_walk.hip — the chunk walks: the first launch of the decode pipeline (overview: rio_place.hip).
//   k_walk          one wave per 32 KiB chunk: speculative entries at every 91 8d 4c candidate,
//                   framed in parallel (readRecordHeaderV4/V3, common_reader.go:83-151; payload
//                   sizing common_reader.go:162-169; snappy preamble = decoded size), chain picked
//                   by a lane vote; records to per-chunk scratch.
//   k_walk_lane     one lane per small chunk: the serial walk with its memory access shaped for a lane.
// Either one also reads the file header (readFileHeaderFromBuffer, common_reader.go:22-44) and its block 0 resets
// ScanState. Both leave the slots and ChunkSums of find_entry + walk_chunk (rio_frame.h), which the scan stitches.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_frame.h"
#include "rio_launch.h"
#include "rio_wave.h"

namespace rio {

// The per-call state reset: block 0's first thread resets the state the later kernels accumulate into (no
// separate launch)
__device__ __forceinline__ void init_state(const FrameParams& P) {
    ScanState* st = P.state;
    const uint8_t* f = P.file;
    st->n_records = 0;
    st->total_bytes = 0;
    st->status = RIO_OK;
    st->status_offset = RIO_FILE_HEADER_BYTES;
    st->det0 = st->det1 = 0;
    st->zero_from = kNone;
    st->zero_nonzero = 0;
    st->n_repairs = 0;
    st->first_bad = kNone;
    st->n_bad = 0;
    st->unsupported_rec = kNone;
    st->n_fail_lanes = 0;
    st->capacity_fail = 0;
    st->huge_streams = 0;
    st->any_mixed = 0;
    st->slow = 0;
    st->scan_ticket = 0;
    st->finish_ticket = 0;
    st->pipe_next = 0;
    st->gz_resize = 0;
    st->gz_redo = 0;
    if (P.len < RIO_FILE_HEADER_BYTES) {
        st->hdr_status = RIO_ERR_SHORT_FILE_HEADER;
        st->version = st->compression = 0;
        return;
    }
    uint32_t v = f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    uint32_t c = f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
    st->version = v;
    st->compression = c;
    int hs = RIO_OK;
    if (v > RIO_VERSION4 || v < RIO_VERSION1) {
        hs = RIO_ERR_VERSION;
        st->det0 = v;
    } else if (c > RIO_COMP_LZW) {
        hs = RIO_ERR_COMPRESSION_TYPE;
        st->det0 = c;
    }
    st->hdr_status = hs;
}

// Cooperative chunk walk: one wave per chunk, processed in windows of up to 64 candidates.
//   1. fill: the wave reads 4 KiB at a time (four 1 KiB coalesced blocks, loads in flight
//      together) and compacts the positions of the canonical magic bytes 91 8d 4c (find_entry's
//      candidates) into LDS in file order, until ~48 are listed or 16 KiB were read; a 65th
//      candidate ends the window exactly at its position (the next window starts there);
//   2. every listed candidate is framed at once (frame_record, one lane each, result in registers);
//   3. the chain is followed with wave votes: the entry is the first candidate that frames
//      (find_entry); a run of candidates chains while each record's successor is the next
//      candidate; a record whose successor skips candidates (magic bytes inside its payload)
//      restarts the vote at its successor. Windows the chain jumps over (long records) are not
//      read. Wherever the chain leaves the candidates (a header that fails, a non-canonical magic
//      encoding) lane 0 takes over with the serial walk (walk_from) for the rest of the chunk.
// Result and slots are identical to find_entry + walk_chunk (the serial thread-per-chunk walk,
// which paid ~50 dependent global round trips per 4 KiB chunk).
constexpr uint32_t kWalkWaves = 4;     // chunks per workgroup
constexpr uint32_t kWalkFill = 56;     // stop filling a window at this many candidates
constexpr uint32_t kWalkFillMax = 8;   // ... or after this many 4 KiB fill rounds

struct WalkLds {
    uint64_t pos[64];
    uint64_t overflow;  // first candidate beyond the 64 listed (kNone if none)
};

// kWalkOcc waves per SIMD at least (rio_device.h, where the measurements behind the value are recorded)
__global__ void __launch_bounds__(64 * kWalkWaves, kWalkOcc) k_walk(FrameParams P) {
    __shared__ WalkLds W[kWalkWaves];
    __shared__ uint32_t crct[1024];
    const uint32_t pf = code_pf(blockIdx.x < kPfBlocks ? kPfWalk : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) init_state(P);
    crc32c_tab_init(crct);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t c = (uint64_t)blockIdx.x * kWalkWaves + wv;
    uint32_t ver, comp;
    if (c >= P.n_chunks || file_header_status(P, ver, comp) != RIO_OK) return;  // wave-uniform
    WalkLds& L = W[wv];
    const uint64_t cs = chunk_start(P, c), ce = chunk_end(P, c);
    const uint8_t* f = P.file;
    WalkSlot* sc = P.scratch + c * P.slots;
    // wave-uniform chain state
    uint64_t p = (c == 0) ? (uint64_t)RIO_FILE_HEADER_BYTES : kNone;  // next record start to chain
    uint32_t mode = (c == 0) ? 1u : 0u;  // 0 entry search, 1 chaining, 2 serial takeover at p
    uint64_t count = 0, bytes = 0, entry = p;
    uint64_t ws = cs;  // window start: candidates are positions >= ws
    while (ws < ce && mode < 2) {
        if (mode == 1) {
            if (p >= ce) break;
            ws = umax(ws, p);  // skip what the chain jumped over
        }
        // 1. fill the window [ws, we)
        if (lane == 0) L.overflow = kNone;
        uint32_t total = 0;
        uint64_t rd = ws & ~15ull;  // next 16-B aligned read position
        // a round that lists no new candidate after some were found ends the fill (long records: the
        // rest of the window would be payload the chain jumps over)
        uint32_t added = 1;
        for (uint32_t r = 0; r < kWalkFillMax && rd < ce && total < kWalkFill && total <= 64 && (total == 0 || added);
             r++) {
            uint4 blk[4];
            uint32_t tail[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t q = rd + 1024 * j + 16 * lane;
                if (q < ce) {  // 16-B aligned; q + 20 <= len + RIO_DEVICE_PAD
                    blk[j] = *reinterpret_cast<const uint4*>(f + q);
                    tail[j] = *reinterpret_cast<const uint32_t*>(f + q + 16);
                }
            }
            uint32_t masks[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t q = rd + 1024 * j + 16 * lane;
                masks[j] = 0;
                if (q < ce) {
                    const uint32_t d[5] = {blk[j].x, blk[j].y, blk[j].z, blk[j].w, tail[j]};
                    masks[j] = magic_mask(d, q, ws, ce, P.len, magic3(ver));
                }
            }
            // list slots of the four blocks' candidates (file order: block j, then lane) from two
            // packed DPP scans (16-bit fields: a block holds at most 1024 candidates)
            const uint32_t c01 = __popc(masks[0]) | (__popc(masks[1]) << 16);
            const uint32_t c23 = __popc(masks[2]) | (__popc(masks[3]) << 16);
            const uint32_t i01 = wave_incl<false>(c01), i23 = wave_incl<false>(c23);
            const uint32_t t01 = lane63(i01), t23 = lane63(i23);
            const uint32_t e01 = i01 - c01, e23 = i23 - c23;
            const uint32_t T0 = t01 & 0xFFFFu, T1 = t01 >> 16, T2 = t23 & 0xFFFFu;
            const uint32_t kb[4] = {total + (e01 & 0xFFFFu), total + T0 + (e01 >> 16), total + T0 + T1 + (e23 & 0xFFFFu),
                                    total + T0 + T1 + T2 + (e23 >> 16)};
            added = T0 + T1 + T2 + (t23 >> 16);
            total += added;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint64_t q = rd + 1024 * j + 16 * lane;
                uint32_t mask = masks[j];
                uint32_t k = kb[j];
                while (mask) {
                    const uint32_t i = __ffs(mask) - 1;
                    mask &= mask - 1;
                    if (k < 64)
                        L.pos[k] = q + i;
                    else if (k == 64)
                        L.overflow = q + i;
                    k++;
                }
            }
            rd += 4096;
        }
        wave_sync_lds();
        const uint64_t overflow = L.overflow;
        const uint64_t we = overflow != kNone ? overflow : umin(rd, ce);  // window end
        // 2. frame one candidate per lane
        const uint32_t nst = umin(total, 64u);
        const bool have = lane < nst;
        const uint64_t cpos = have ? L.pos[lane] : kNone;
        Hdr h;
        h.nil = false;
        uint64_t nx = 0, ol = 0, pd = 0, lf = 0;
        int e = RIO_ERR_MAGIC;
        if (have) e = frame_record(f, P.len, cpos, ver, comp, h, nx, ol, pd, lf, crct);
        const bool ok = have && e == RIO_OK;
        const uint64_t ok_mask = __ballot(ok);
        const uint64_t succ_pos = __shfl_down(cpos, 1);  // next candidate's position
        // 3. entry and chain by votes
        if (mode == 0) {
            const uint32_t k = lane_ffs(ok_mask);
            if (k < 64) {
                p = readlane64(cpos, k);
                mode = 1;
            }
            entry = p;
        }
        uint32_t slot = ~0u;
        while (mode == 1 && p < we) {
            // the candidate at p, if listed and framed
            const uint32_t e0 = lane_ffs(__ballot(have && cpos >= p));
            if (e0 >= nst || readlane64(cpos, e0) != p || !((ok_mask >> e0) & 1)) {
                mode = 2;  // serial takeover at p
                break;
            }
            // maximal run e0..b where each record's successor is the next candidate
            const bool link = ok && lane + 1 < nst && nx == succ_pos;
            const uint64_t brk = ~__ballot(link) & (~0ull << e0);
            const uint32_t b = lane_ffs(brk);  // first non-linking candidate (< nst: lane nst-1 never links)
            // b is reached by the chain; if its header fails, the chain stops AT it (serial takeover
            // classifies the error), else b is the run's last record
            const bool bok = (ok_mask >> b) & 1;
            const uint32_t last = bok ? b : b - 1;  // b > e0 when !bok (e0 frames)
            if (lane >= e0 && lane <= last) slot = (uint32_t)count + (lane - e0);
            count += last - e0 + 1;
            p = bok ? readlane64(nx, b) : readlane64(cpos, b);
        }
        // 4. scratch slots of the chained candidates + their decoded bytes
        const uint64_t mylen = slot != ~0u ? ol : 0;
        if (slot != ~0u && slot < P.slots) slot_store(sc + slot, cpos - cs, ol | lf | (h.nil ? kNilBit : 0), pd);
        uint64_t wsum;
        wave_excl_scan64(mylen, lane, wsum);
        bytes += wsum;
        wave_sync_lds();
        ws = we;
    }
    // 5. serial takeover where the chain left the candidates; the chunk summary
    if (lane == 0) {
        ChunkSum s = chunk_sum_empty(entry);
        s.count = (uint32_t)count;
        s.bytes = bytes;
        if (mode == 2)
            walk_from(P, c, p, ver, comp, s);
        else if (entry != kNone)
            s.exit = p;  // the chain left the chunk (or ended at the file end) cleanly
        P.chunks[c] = s;
    }
    code_pf_done(pf);
}

// ------------------------------------------------------------------------------------------
// Lane walk (round 5, RIO_WALK_LANE): one LANE per chunk (small chunks, 16 KiB by default, RIO_LANE_CHUNK_BYTES), the serial
// FileReader walk of find_entry + walk_chunk with the memory access shaped for a lane:
//   * entry search: 64 bytes per step as four aligned 16-byte loads issued together (plus the next
//     dword), candidates from magic_mask (0x91 bytes, then the 3-byte test), each framed by
//     frame_record; the first that frames is the chunk's speculative entry (as find_entry);
//   * then header to header: each hop is ONE round trip (two 16-byte loads at the header, issued as soon as the
//     previous header's lengths are known; the header verified in registers under them, CRC-32C from the LDS
//     slice-by-4 table) and the payload is never read.
// Slots and ChunkSum are the serial walk's, so the scan, the repair and the placement are unchanged.
// Against the wave-per-chunk walk (k_walk) it reads ~64 bytes per record instead of every byte, and
// its framing work is per record, not per candidate window. Its cost per record per lane is the hop's own
// instructions at one wave per SIMD (1.9 of 2.2 us on C2) more than the round trip (profiles/r15/r15a_lane_hops_probe.txt).
// ------------------------------------------------------------------------------------------
// A framed record as the walk keeps it: the next record's start and the slot's fields
struct LaneRec {
    uint64_t next, olen, pd, lf;
    bool nil;
};

// ver / comp: compile-time constants in k_walk_lane's v4 instantiations, the file's values in the generic one. A chunk's
// entry comes back framed (r), so the walk's first action is the load at r.next.
__device__ __forceinline__ uint64_t find_entry_lane(const FrameParams& P, uint64_t cs, uint64_t ce, uint32_t ver,
                                                    uint32_t comp, const uint32_t* crct, LaneRec& r) {
    const uint8_t* f = P.file;
    const uint32_t m3 = magic3(ver);
    // a whole 128-byte line per step (8 loads, the next dword too), the next line loaded before this one's candidates are
    // tested: two steps in flight. Round 6: the entry search was a chain of dependent 64-byte steps, ~3.5 us each under
    // the walk's load (probe build), C2-ref-random walk 0.129 -> 0.117 ms (profiles/r6/r6r_lane_walk_entry.txt). The nine
    // loads go out without a branch each: an address at or past the file end is clamped to the file's last aligned block
    // (the device pad covers 64 bytes only), whose bytes stand in for positions magic_mask never lists (i + 2 < len - q).
    const uint64_t last16 = (P.len - 1) & ~15ull, last4 = (P.len - 1) & ~3ull;  // len >= the file header's 8 bytes
    auto fetch = [&](uint64_t q, uint4 (&v)[8], uint32_t& t) __attribute__((always_inline)) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) v[j] = *reinterpret_cast<const uint4*>(f + umin(q + 16 * j, last16));
        t = *reinterpret_cast<const uint32_t*>(f + umin(q + 128, last4));
    };
    uint64_t q0 = cs & ~127ull;
    uint4 a[8];
    uint32_t t;
    fetch(q0, a, t);
    for (;;) {
        const uint64_t q1 = q0 + 128;
        uint4 na[8];
        uint32_t nt = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) na[j] = zero4();
        if (q1 < ce) fetch(q1, na, nt);
        // candidate bits of the line's 128 positions (static indices only: the blocks stay in registers)
        uint64_t mlo = 0, mhi = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t nx = j < 7 ? a[j + 1].x : t;
            const uint32_t d[5] = {a[j].x, a[j].y, a[j].z, a[j].w, nx};
            const uint64_t m = (uint64_t)magic_mask(d, q0 + 16 * j, cs, ce, P.len, m3) << (16 * (j & 3));
            if (j < 4)
                mlo |= m;
            else
                mhi |= m;
        }
        while (mlo | mhi) {
            const bool lo = mlo != 0;
            const uint64_t mm = lo ? mlo : mhi;
            const uint64_t p = q0 + (lo ? 0u : 64u) + (uint64_t)__builtin_ctzll(mm);
            if (lo)
                mlo &= mlo - 1;
            else
                mhi &= mhi - 1;
            // frame_record on the candidate, kept framed for the walk. Its 32 bytes are loaded again: taken from the two
            // lines held by static-index selects (~120 VALU per candidate, the whole wave's) the search was slower, entry
            // 23.0 -> 26.1 us per lane and C2 walk 0.093 -> 0.097 ms (profiles/r15/r15a_lane_hops_ab.txt, "inreg")
            Hdr hd;
            int e = kFrameSlow;
            r.lf = 0;
            if (p + 32 <= P.len) {
                const uint4 x = ldu16(f + p), y = ldu16(f + p + 16);
                const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                FastLen L;
                if (frame_lengths(w, P.len, p, ver, comp, L) && frame_verify(w, L, ver, comp, hd, r.olen, r.pd, crct)) {
                    r.next = L.next;
                    e = RIO_OK;
                }
            }
            if (e != RIO_OK) e = frame_slow(f, P.len, p, ver, comp, hd, r.next, r.olen, r.pd, r.lf);
            if (e == RIO_OK) {
                r.nil = hd.nil;
                return p;
            }
        }
        if (q1 >= ce) return kNone;
        q0 = q1;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) a[j] = na[j];
        t = nt;
    }
}

// walk_from for one lane: the same records, slots and summary. A hop is one load round trip and nothing else in
// series with it that the next address does not need: frame_lengths gives the next record's start, the two loads at it
// go out once it has passed the walk's bounds (next < ce && next + 32 <= len; next <= len by frame_lengths), and the
// CRC-32C, the snappy preamble and the slot store run under them. A record that then fails frame_verify takes
// frame_slow exactly as one that fails frame_fast: the loaded bytes are dropped and no slot is stored behind it. The
// loads precede the slot store (on CDNA vmcnt retires loads and stores in issue order: a load issued after the store
// would wait for it too). The slot is one 16-byte store: a wave's lanes write 64 different lines per store
// instruction, and three 8-byte stores per record were two thirds of the kernel's memory requests.
// framed: the record at p is the entry search's (r), else it is framed here first.
__device__ __forceinline__ void walk_from_lane(const FrameParams& P, uint64_t c, uint64_t p, bool framed, LaneRec r,
                                               uint32_t ver, uint32_t comp, ChunkSum& s, const uint32_t* crct) {
    const uint8_t* f = P.file;
    const uint64_t cs = chunk_start(P, c), ce = chunk_end(P, c);
    WalkSlot* sc = P.scratch + c * P.slots;
    bool have = !framed && p < ce && p + 32 <= P.len;
    uint4 a = zero4(), b = zero4();
    if (have) {
        a = ldu16(f + p);
        b = ldu16(f + p + 16);
    }
    while (p < ce) {
        bool loaded = false;  // the loads at r.next are out (or next is known to have no window)
        if (!framed) {
            Hdr h;
            int e = kFrameSlow;
            r.lf = 0;
            if (have) {
                const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                FastLen L;
                if (frame_lengths(w, P.len, p, ver, comp, L)) {
                    have = L.next < ce && L.next + 32 <= P.len;
                    if (have) {
                        a = ldu16(f + L.next);
                        b = ldu16(f + L.next + 16);
                    }
                    if (frame_verify(w, L, ver, comp, h, r.olen, r.pd, crct)) {
                        r.next = L.next;
                        loaded = true;
                        e = RIO_OK;
                    }
                }
            }
            if (e != RIO_OK) e = frame_slow(f, P.len, p, ver, comp, h, r.next, r.olen, r.pd, r.lf);
            if (e) {
                s.status = e;
                s.err_off = p;
                if (e == RIO_ERR_HEADER_CRC) {
                    s.det0 = h.exp_crc;
                    s.det1 = h.act_crc;
                } else if (e == RIO_ERR_MAGIC) {
                    s.det0 = h.magic_len;
                } else if (e == RIO_ERR_UNEXPECTED_EOF && h.hdr_len != 0) {
                    s.det0 = 1;  // raised by the payload read, not by a header varint
                }
                break;
            }
            r.nil = h.nil;
        }
        framed = false;
        if (!loaded) {
            have = r.next < ce && r.next + 32 <= P.len;
            if (have) {
                a = ldu16(f + r.next);
                b = ldu16(f + r.next + 16);
            }
        }
        if (s.count < P.slots) slot_store(sc + s.count, p - cs, r.olen | r.lf | (r.nil ? kNilBit : 0), r.pd);
        s.count++;
        s.bytes += r.olen;
        p = r.next;
    }
    s.exit = s.status ? s.err_off : p;
}

// One lane's chunk: entry search, walk, summary
__device__ __forceinline__ void lane_chunk(const FrameParams& P, uint64_t c, uint32_t ver, uint32_t comp,
                                           const uint32_t* crct) {
    const uint64_t cs = chunk_start(P, c), ce = chunk_end(P, c);
    LaneRec r{0, 0, 0, 0, false};
    const uint64_t from = c == 0 ? (uint64_t)RIO_FILE_HEADER_BYTES : find_entry_lane(P, cs, ce, ver, comp, crct, r);
    ChunkSum s = chunk_sum_empty(from);
    if (from != kNone) walk_from_lane(P, c, from, c != 0, r, ver, comp, s, crct);
    P.chunks[c] = s;
}

// Lanes per workgroup of k_walk_lane (a multiple of 64; every wave takes its share of the 4 KiB CRC table's copy). 64
// spreads C2's 535 waves over every CU where 256 holds them on 134 of the 256: C2 walk 0.095 -> 0.089 ms in five of five
// rounds, but the decode stage behind it measured 0.006 ms longer in the same rounds and the value the same (472.1
// against 471.6 GiB/s), and C2-ref-random walked 0.095 -> 0.101 ms: 256 stays (profiles/r15/r15a_lane_hops_ab.txt,
// lines "inreg" = 256 lanes and "wg64").
constexpr uint32_t kWalkLaneBlock = 256;
__global__ void __launch_bounds__(kWalkLaneBlock) k_walk_lane(FrameParams P) {
    __shared__ uint32_t crct[1024];
    if (blockIdx.x == 0 && threadIdx.x == 0) init_state(P);
    for (uint32_t i = threadIdx.x; i < 256; i += kWalkLaneBlock)
        reinterpret_cast<uint4*>(crct)[i] = reinterpret_cast<const uint4*>(kCrc32c.t)[i];
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * kWalkLaneBlock + threadIdx.x;
    uint32_t ver, comp;
    if (c >= P.n_chunks || file_header_status(P, ver, comp) != RIO_OK) return;
    // the file's version and codec are wave-uniform: v4 files without compression and with snappy walk through
    // instantiations where both are constants, every other file through the generic code
    if (ver == RIO_VERSION4 && comp == RIO_COMP_NONE)
        lane_chunk(P, c, RIO_VERSION4, RIO_COMP_NONE, crct);
    else if (ver == RIO_VERSION4 && comp == RIO_COMP_SNAPPY)
        lane_chunk(P, c, RIO_VERSION4, RIO_COMP_SNAPPY, crct);
    else
        lane_chunk(P, c, ver, comp, crct);
}

// The walk's launch: k_walk_lane when the context chose the lane walk for this file (P.walk_lane), else k_walk.
// start / stop: the stage events (either may be null)
void launch_walk(const FrameParams& P, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    if (P.walk_lane)
        launch_ev(k_walk_lane, dim3(blocks_for(P.n_chunks, kWalkLaneBlock)), dim3(kWalkLaneBlock), s, start, stop, P);
    else
        launch_ev(k_walk, dim3(blocks_for(P.n_chunks, kWalkWaves)), dim3(64 * kWalkWaves), s, start, stop, P);
}

}  // namespace rio
