// rio_frame.h — what every framing consumer needs to frame one record and walk one chunk serially:
// the code prefetch, CRC-32C, the record header parse (byte-wise and from a 32-byte register window), frame_record
// and its halves, the file header, chunk bounds and magic candidates, and the serial chunk walk with its slots.
// Shared by the walks (rio_walk.hip), the scan's repair (rio_chunk_scan.hip), placement (rio_place.hip) and the
// single-record / index kernels (rio_seek.hip). Byte/integer work only; all offsets 64-bit.
// Included by .hip files only. Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_pb.h"

namespace rio {

// Code prefetch: after a MALL flush a launch's instruction fetches come from HBM one
// 64-byte line at a time, a dependent miss chain through the kernel's straight-line code (round 6 probe: the
// scan's cold chain 36 -> 31 us with the next 4 KiB of its code read as data at entry, profiles/r6/
// r6k_small_file_framing.txt). Lane t < lines of the calling wave loads the dword at pc + 64 t into L2 (one line
// each; the SQC's misses then hit L2); code_pf_done consumes the value where the wave waits anyway. `lines` stays
// within the kernel's own code: tests/test_kernel_lint.py checks every prefetching kernel against the code object.
__device__ __forceinline__ uint32_t code_pf(uint32_t lines) {
    uint32_t v = 0;
    if (threadIdx.x < lines)
        v = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(__builtin_amdgcn_s_getpc() +
                                                                                  64u * threadIdx.x);
    return v;
}
__device__ __forceinline__ void code_pf_done(uint32_t v) {
    asm volatile("" ::"v"(v));
}
// lines per kernel (tests/test_kernel_lint.py: within each kernel's own code); the wide grids prefetch from their first
// 16 blocks only (two per XCD: each XCD's L2 then holds the code)
constexpr uint32_t kPfScan = 64, kPfPlace = 48, kPfCopy = 64, kPfFinish = 64, kPfWalk = 64, kPfBlocks = 16;

// ------------------------------------------------------------------------------------------
// Byte-level primitives
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t crc32c_byte(uint32_t c, uint32_t b) {
    c ^= b;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
    return c;
}

// Byte sources for the header / scan code: RawBytes reads the file directly; WinBytes (rio_pb.h)
// serves a lane's bytes from a 16-byte window and reloads it only when a position leaves it.
// io.ByteReader over file bytes [base, base+avail); `cap` = checksumByteReader cache (36 for v4
// FileReader, checksum_byte_reader.go:25-27), ~0 when no cache applies.
template <class B>
struct SrcT {
    B& get;
    uint64_t base, avail, pos, cap;
};

template <class B>
__device__ __forceinline__ int src_byte(SrcT<B>& s, uint32_t& b) {
    if (s.pos >= s.avail) return RIO_EOF;
    if (s.pos >= s.cap) {
        s.pos++;
        return RIO_ERR_HEADER_TOO_LONG;
    }
    b = s.get(s.base + s.pos++);
    return RIO_OK;
}

// encoding/binary.ReadUvarint semantics
template <class B>
__device__ __forceinline__ int read_uvarint(SrcT<B>& s, uint64_t& x) {
    uint64_t v = 0;
    uint32_t sh = 0;
    for (int i = 0; i < 10; i++) {
        uint32_t b;
        int e = src_byte(s, b);
        if (e) return (e == RIO_EOF && i > 0) ? RIO_ERR_UNEXPECTED_EOF : e;
        if (b < 0x80) {
            if (i == 9 && b > 1) return RIO_ERR_VARINT_OVERFLOW;
            x = v | ((uint64_t)b << sh);
            return RIO_OK;
        }
        v |= (uint64_t)(b & 0x7F) << sh;
        sh += 7;
    }
    return RIO_ERR_VARINT_OVERFLOW;
}

// uvarint_buf (rio_dev_util.h: encoding/binary.Uvarint) over bytes [p, p + n) of a byte source
template <class B>
__device__ __forceinline__ int uvarint_at(B& get, uint64_t p, uint64_t n, uint64_t& x) {
    uint64_t v = 0;
    uint32_t sh = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (i == 10) return -(int)(i + 1);
        const uint32_t b = get(p + i);
        if (b < 0x80) {
            if (i == 9 && b > 1) return -(int)(i + 1);
            x = v | ((uint64_t)b << sh);
            return (int)(i + 1);
        }
        v |= (uint64_t)(b & 0x7F) << sh;
        sh += 7;
    }
    return 0;
}

// The preamble of the Snappy payload at [pay, pay + plen) by ReadNextAt's rule (read_at_dev, rio_seek.hip): false
// (ErrCorrupt) for an unusable varint, a length past 32 bits, or one above 22x the element bytes + 64; else its k
// bytes and the decoded length
template <class B>
__device__ __forceinline__ bool snappy_preamble_at(B& get, uint64_t pay, uint64_t plen, uint32_t& k, uint64_t& dl) {
    dl = 0;
    const int kk = uvarint_at(get, pay, plen, dl);
    k = kk > 0 ? (uint32_t)kk : 0u;
    return kk > 0 && dl <= 0xFFFFFFFFull && dl <= 22ull * (plen - (uint64_t)kk) + 64;
}

struct Hdr {
    uint64_t u, c, exp_crc, act_crc;
    uint32_t hdr_len, magic_len;
    int nil;
};

__device__ __forceinline__ int later_field(int e) { return e == RIO_EOF ? RIO_EOF_HEADER : e; }

// readRecordHeaderV4 (common_reader.go:110-151) / readRecordHeaderV3 (:83-108) / readRecordHeaderV2
// (:61-81: no nil byte, no CRC)
template <class B>
__device__ __forceinline__ int parse_header_t(B& get, uint64_t p, uint64_t avail, uint64_t cap, uint32_t ver, Hdr& h,
                                              const uint32_t* crc_tab = nullptr) {
    h.nil = 0;
    h.hdr_len = 0;
    if (ver == RIO_VERSION1) {
        // readRecordHeaderV1 (common_reader.go:46-59) after io.ReadFull of 20 bytes (file_reader.go:282-293):
        // nothing left -> io.EOF, a partial header -> io.ErrUnexpectedEOF; no zero-tail rule
        h.magic_len = 0;
        if (avail == 0) return RIO_EOF;
        if (avail < RIO_RECORD_HEADER_V1_BYTES) return RIO_ERR_UNEXPECTED_EOF;
        uint32_t m = 0;
        uint64_t u = 0, c = 0;
        for (uint32_t i = 0; i < 4; i++) m |= (uint32_t)get(p + i) << (8 * i);
        if (m != RIO_MAGIC) return RIO_ERR_MAGIC;
        for (uint32_t i = 0; i < 8; i++) {
            u |= (uint64_t)get(p + 4 + i) << (8 * i);
            c |= (uint64_t)get(p + 12 + i) << (8 * i);
        }
        h.u = u;
        h.c = c;
        h.hdr_len = RIO_RECORD_HEADER_V1_BYTES;
        return RIO_OK;
    }
    SrcT<B> s{get, p, avail, 0, cap};
    uint64_t m = 0;
    int e = read_uvarint(s, m);
    h.magic_len = (uint32_t)s.pos;
    if (e) return e;
    if (m != RIO_MAGIC) return RIO_ERR_MAGIC;
    uint32_t nb = 0;
    if (ver >= RIO_VERSION3) {
        e = src_byte(s, nb);
        if (e) return later_field(e);
    }
    e = read_uvarint(s, h.u);
    if (e) return later_field(e);
    e = read_uvarint(s, h.c);
    if (e) return later_field(e);
    if (ver == RIO_VERSION4) {
        uint32_t crc = 0xFFFFFFFFu;
        // byte table in LDS when the kernel has one (T[0..255] of crc32c_tab_init), else bitwise
        if (crc_tab)
            for (uint64_t i = 0; i < s.pos; i++) crc = crc_tab[(crc ^ get(p + i)) & 0xFFu] ^ (crc >> 8);
        else
            for (uint64_t i = 0; i < s.pos; i++) crc = crc32c_byte(crc, get(p + i));
        h.act_crc = crc ^ 0xFFFFFFFFu;
        e = read_uvarint(s, h.exp_crc);
        if (e) return later_field(e);
        if (h.act_crc != h.exp_crc) return RIO_ERR_HEADER_CRC;
    }
    h.nil = (nb == 1);
    h.hdr_len = (uint32_t)s.pos;
    return RIO_OK;
}

__device__ __forceinline__ int parse_header(const uint8_t* f, uint64_t p, uint64_t avail, uint64_t cap, uint32_t ver,
                                            Hdr& h) {
    RawBytes raw{f};
    return parse_header_t(raw, p, avail, cap, ver, h);
}

// ---- register-window header parse (fast path) --------------------------------------------
// 8 bytes starting at byte k (0..23: dwords j .. j + 2 with j <= 5) of a 32-byte window held in 8 dwords
__device__ __forceinline__ uint64_t win8(const uint32_t (&w)[8], uint32_t k) {
    const uint32_t j = k >> 2, r = 8 * (k & 3);
    uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
#pragma unroll
    for (uint32_t t = 1; t < 6; t++) {
        d0 = j == t ? w[t] : d0;
        d1 = j == t ? w[t + 1] : d1;
        d2 = j == t ? w[t + 2] : d2;
    }
    const uint64_t a = ((uint64_t)d1 << 32) | d0, b = d2;
    return r ? (a >> r) | (b << (64 - r)) : a;
}

// 7-bit groups of the four bytes of x packed (LEB128 payload bits of bytes 0..3)
__device__ __forceinline__ uint32_t leb_pack4(uint32_t x) {
    return (x & 0x7Fu) | ((x >> 1) & 0x3F80u) | ((x >> 2) & 0x1FC000u) | ((x >> 3) & 0x0FE00000u);
}

// LEB128 of at most 8 bytes at the bottom of x: returns the byte count (0 if longer than 8)
__device__ __forceinline__ uint32_t varint8(uint64_t x, uint64_t& v) {
    const uint64_t stop = ~x & 0x8080808080808080ull;
    const uint32_t nb = stop ? (__builtin_ctzll(stop) >> 3) + 1 : 0u;
    const uint64_t y = x & (nb >= 8 || nb == 0 ? ~0ull : ((1ull << (8 * nb)) - 1));
    // two 32-bit halves of 28 payload bits each (the 64-bit group loop cost ~45 VALU per call)
    const uint32_t lo = leb_pack4((uint32_t)y), hi = leb_pack4((uint32_t)(y >> 32));
    v = ((uint64_t)hi << 28) | lo;
    return nb;
}

__device__ __forceinline__ uint32_t crc32c_bytes(uint32_t c, uint64_t x, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) c = crc32c_byte(c, (uint32_t)(x >> (8 * i)) & 0xFF);
    return c;
}

// CRC-32C register state after the canonical magic bytes 91 8d 4c (before the final xor)
__device__ __forceinline__ uint32_t crc_after_magic() {
    uint32_t c = 0xFFFFFFFFu;
    c = crc32c_byte(c, 0x91);
    c = crc32c_byte(c, 0x8D);
    return crc32c_byte(c, 0x4C);
}

// CRC-32C slice-by-4 over LDS tables T[0..1023] (T0..T3, reflected polynomial 0x82F63B78):
// n <= 16 bytes given little-endian in x0 (bytes 0..7) and x1 (bytes 8..15). Register state in/out.
__device__ __forceinline__ uint32_t crc32c_tab(uint32_t c, uint64_t x0, uint64_t x1, uint32_t n, const uint32_t* T) {
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = c ^ (uint32_t)((i < 8 ? x0 >> (8 * i) : x1 >> (8 * (i - 8))));
        c = T[768 + (w & 0xFF)] ^ T[512 + ((w >> 8) & 0xFF)] ^ T[256 + ((w >> 16) & 0xFF)] ^ T[w >> 24];
    }
    for (; i < n; i++) {
        const uint32_t b = (uint32_t)((i < 8 ? x0 >> (8 * i) : x1 >> (8 * (i - 8)))) & 0xFF;
        c = T[(c ^ b) & 0xFF] ^ (c >> 8);
    }
    return c;
}

// The slice-by-4 tables, computed at compile time (CRC-32C, reflected polynomial 0x82F63B78)
struct Crc32cTables {
    uint32_t t[1024];
    constexpr Crc32cTables() : t() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
            t[i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (uint32_t k = 1; k < 4; k++) t[256 * k + i] = (t[256 * (k - 1) + i] >> 8) ^ t[t[256 * (k - 1) + i] & 0xFF];
    }
};
// Defined in a header and built without relocatable device code: every code object that uses the table holds its own
// 4 KiB copy.
__device__ const Crc32cTables kCrc32c{};

// Copy the slice-by-4 tables into LDS (blockDim.x >= 256: one 16-byte piece per thread; round 4:
// a load instead of ~45 VALU per thread of bitwise table building); ends with a workgroup barrier.
// static, without the inline hint the other functions of this header carry: the hint pulls it into k_index_search,
// whose registers and spills are tuned with this call out of line (rio_seek.hip)
static __device__ void crc32c_tab_init(uint32_t* T) {
    const uint32_t i = threadIdx.x;
    if (i < 256) reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(kCrc32c.t)[i];
    __syncthreads();
}

// lzw records are sized by the header's u (the reference's buffer size, the decoded length for every
// file its writer produces) while an lzw stream of `plen` bytes can reach it: a 9-bit code expands to
// at most 4096 bytes (oracle ORC_LZW_MAX_RATIO). k_lzw_decode counts and re-places any other size.
__device__ __forceinline__ uint64_t lzw_size(uint64_t u, uint64_t plen) { return u <= 4096ull * plen ? u : 0; }

// The fast path of frame_record on the 32 bytes at p already in registers (w; p + 32 <= len): RIO_OK
// with the record framed (lflags 0), or kFrameSlow when the record needs the byte-wise path below.
constexpr int kFrameSlow = -1000;
__device__ __forceinline__ int frame_fast(const uint32_t (&w)[8], uint64_t len, uint64_t p, uint32_t ver, uint32_t comp,
                                          Hdr& h, uint64_t& next, uint64_t& out_len, uint64_t& pay,
                                          const uint32_t* crct) {
    const uint4 a = make_uint4(w[0], w[1], w[2], w[3]), b = make_uint4(w[4], w[5], w[6], w[7]);
    {
        if (ver == RIO_VERSION1 ? a.x == RIO_MAGIC : (a.x & 0xFFFFFFu) == 0x4C8D91u) {
            // v3 / v4: the nil byte at 3, the sizes from 4; v2: no nil byte (readRecordHeaderV2)
            // v1: fixed 20 bytes, LE u64 sizes at 4 and 12 (readRecordHeaderV1)
            const uint32_t hb = ver >= RIO_VERSION3 ? 4u : 3u;
            uint64_t u = 0, c = 0, crc = 0;
            uint32_t nu, nc;
            if (ver == RIO_VERSION1) {
                u = ((uint64_t)a.z << 32) | a.y;
                c = ((uint64_t)b.x << 32) | a.w;
                nu = 8;
                nc = 9;  // hb (3) + 8 + 9 = 20
            } else {
                nu = varint8(win8(w, hb), u);
                nc = nu ? varint8(win8(w, hb + nu), c) : 0;
            }
            uint32_t hl = hb + nu + nc;
            bool ok = nu && nc;
            uint32_t act = 0;
            if (ok && ver == RIO_VERSION4) {
                const uint32_t ncrc = varint8(win8(w, hl), crc);
                uint32_t cs;
                if (crct && nu + nc <= 15) {  // nil byte + both varints: bytes [3, 4 + nu + nc)
                    cs = crc32c_tab(crc_after_magic(), win8(w, 3), win8(w, 11), 1 + nu + nc, crct);
                } else {
                    cs = crc32c_byte(crc_after_magic(), (a.x >> 24) & 0xFF);
                    cs = crc32c_bytes(cs, win8(w, 4), nu);
                    cs = crc32c_bytes(cs, win8(w, 4 + nu), nc);
                }
                act = cs ^ 0xFFFFFFFFu;
                ok = ncrc && act == crc;
                hl += ncrc;
            }
            if (ok) {
                const bool nil = ver >= RIO_VERSION3 && ((a.x >> 24) & 0xFF) == 1;
                const uint64_t plen = comp != RIO_COMP_NONE ? c : u;
                const uint64_t avail = len - p - hl;
                uint64_t dl = plen;
                uint32_t k = 0;
                if (!nil && comp == RIO_COMP_SNAPPY && hl <= 20) {  // win8 covers k <= 20 with 8 bytes inside the window
                    k = varint8(win8(w, hl), dl);
                    ok = k && k <= plen && dl <= 0xFFFFFFFFull && dl <= 22ull * (plen - k) + 64;
                } else if (!nil && comp == RIO_COMP_LZW) {
                    dl = lzw_size(u, plen);
                } else if (!nil && comp != RIO_COMP_NONE) {
                    ok = false;  // snappy preamble outside the window; gzip: sized by its trailer
                }
                if (ok && (nil || plen <= avail)) {
                    h.u = u;
                    h.c = c;
                    h.exp_crc = crc;
                    h.act_crc = act;
                    h.hdr_len = hl;
                    h.magic_len = ver == RIO_VERSION1 ? 0 : 3;
                    h.nil = nil;
                    if (nil) {  // file_reader.go:96-99: nil => no payload bytes
                        next = p + hl;
                        out_len = 0;
                        pay = hl;
                    } else {
                        next = p + hl + plen;
                        out_len = dl;
                        pay = ((plen - k) << 8) | (hl + k);
                    }
                    return RIO_OK;
                }
            }
        }
    }
    return kFrameSlow;
}

// frame_fast in two halves for the lane walk, whose hop waits on one load per record: the lengths (all that the next
// record's address needs) first, the verification under that load. frame_lengths && frame_verify frames exactly the
// records frame_fast frames, with the same results; a record that either half refuses takes frame_slow.
struct FastLen {
    uint64_t u, c, crc, plen, next;
    uint32_t nu, nc, hl;  // hl: the whole header, the CRC varint included
    bool nil;
};
// Magic, nil byte, u, c and the length of the CRC varint of the 32 bytes at p (p + 32 <= len). True: L.next is the next
// record's start and lies in the file (next <= len: plen is compared with the bytes left, never added first, so no
// length can wrap it).
__device__ __forceinline__ bool frame_lengths(const uint32_t (&w)[8], uint64_t len, uint64_t p, uint32_t ver, uint32_t comp,
                                              FastLen& L) {
    if (!(ver == RIO_VERSION1 ? w[0] == RIO_MAGIC : (w[0] & 0xFFFFFFu) == 0x4C8D91u)) return false;
    const uint32_t hb = ver >= RIO_VERSION3 ? 4u : 3u;
    L.u = L.c = L.crc = 0;
    if (ver == RIO_VERSION1) {
        L.u = ((uint64_t)w[2] << 32) | w[1];
        L.c = ((uint64_t)w[4] << 32) | w[3];
        L.nu = 8;
        L.nc = 9;  // hb (3) + 8 + 9 = 20
    } else {
        L.nu = varint8(win8(w, hb), L.u);
        L.nc = L.nu ? varint8(win8(w, hb + L.nu), L.c) : 0;
    }
    if (!(L.nu && L.nc)) return false;
    L.hl = hb + L.nu + L.nc;
    if (ver == RIO_VERSION4) {
        const uint32_t ncrc = varint8(win8(w, L.hl), L.crc);
        if (!ncrc) return false;
        L.hl += ncrc;
    }
    L.nil = ver >= RIO_VERSION3 && ((w[0] >> 24) & 0xFF) == 1;
    L.plen = comp != RIO_COMP_NONE ? L.c : L.u;
    if (!L.nil) {
        // snappy: win8 reaches the preamble only while hl <= 20; gzip is sized by its trailer (frame_slow)
        if (comp == RIO_COMP_SNAPPY ? L.hl > 20 : (comp != RIO_COMP_NONE && comp != RIO_COMP_LZW)) return false;
        if (L.plen > len - p - L.hl) return false;  // hl < 32 <= len - p
    }
    L.next = p + L.hl + (L.nil ? 0 : L.plen);
    return true;
}
// The header CRC-32C, the snappy preamble and its bounds of a record frame_lengths accepted; fills h, out_len, pay.
__device__ __forceinline__ bool frame_verify(const uint32_t (&w)[8], const FastLen& L, uint32_t ver, uint32_t comp, Hdr& h,
                                             uint64_t& out_len, uint64_t& pay, const uint32_t* crct) {
    uint32_t act = 0;
    if (ver == RIO_VERSION4) {
        uint32_t cs;
        if (crct && L.nu + L.nc <= 15) {  // nil byte + both varints: bytes [3, 4 + nu + nc)
            cs = crc32c_tab(crc_after_magic(), win8(w, 3), win8(w, 11), 1 + L.nu + L.nc, crct);
        } else {
            cs = crc32c_byte(crc_after_magic(), (w[0] >> 24) & 0xFF);
            cs = crc32c_bytes(cs, win8(w, 4), L.nu);
            cs = crc32c_bytes(cs, win8(w, 4 + L.nu), L.nc);
        }
        act = cs ^ 0xFFFFFFFFu;
        if (act != L.crc) return false;
    }
    uint64_t dl = L.plen;
    uint32_t k = 0;
    if (!L.nil && comp == RIO_COMP_SNAPPY) {
        k = varint8(win8(w, L.hl), dl);
        if (!(k && k <= L.plen && dl <= 0xFFFFFFFFull && dl <= 22ull * (L.plen - k) + 64)) return false;
    } else if (!L.nil && comp == RIO_COMP_LZW) {
        dl = lzw_size(L.u, L.plen);
    }
    h.u = L.u;
    h.c = L.c;
    h.exp_crc = L.crc;
    h.act_crc = act;
    h.hdr_len = L.hl;
    h.magic_len = ver == RIO_VERSION1 ? 0 : 3;
    h.nil = L.nil;
    if (L.nil) {  // file_reader.go:96-99: nil => no payload bytes
        out_len = 0;
        pay = L.hl;
    } else {
        out_len = dl;
        pay = ((L.plen - k) << 8) | (L.hl + k);
    }
    return true;
}

// The byte-wise path of frame_record (ReadUvarint restatement): every record the fast path does not take,
// and every failure's exact classification.
__device__ inline int frame_slow(const uint8_t* f, uint64_t len, uint64_t p, uint32_t ver, uint32_t comp, Hdr& h,
                          uint64_t& next, uint64_t& out_len, uint64_t& pay, uint64_t& lflags) {
    lflags = 0;
    uint64_t cap = ver == RIO_VERSION4 ? RIO_RECORD_HEADER_V4_MAX : ~0ull;
    int e = parse_header(f, p, len - p, cap, ver, h);
    if (e) return e;
    if (h.nil) {  // file_reader.go:96-99: nil => no payload bytes
        next = p + h.hdr_len;
        out_len = 0;
        pay = h.hdr_len;
        return RIO_OK;
    }
    uint64_t plen = comp != RIO_COMP_NONE ? h.c : h.u;
    uint64_t avail = len - p - h.hdr_len;
    if (plen > avail) return avail == 0 ? RIO_EOF_PAYLOAD : RIO_ERR_UNEXPECTED_EOF;
    uint64_t k = 0;
    next = p + h.hdr_len + plen;
    if (comp == RIO_COMP_SNAPPY) {
        uint64_t d = 0;
        const int kk = uvarint_buf(f + p + h.hdr_len, plen, d);
        // snappy decodedLen: n<=0 or > 0xffffffff => ErrCorrupt; a preamble above 22x the element
        // bytes cannot be produced (max 64 output bytes per 3-byte tagCopy2) => ErrCorrupt later.
        if (kk <= 0 || d > 0xFFFFFFFFull || d > 22ull * (plen - (uint64_t)kk) + 64) {
            out_len = 0;
            pay = h.hdr_len;
            lflags = kBadBit;
            return RIO_OK;
        }
        out_len = d;
        k = (uint64_t)kk;
    } else if (comp == RIO_COMP_GZIP) {
        // gzip.NewReader on an empty payload returns a bare io.EOF, which ReadNext passes through
        // unwrapped (file_reader.go:118-121, gzip_compression.go:56-59)
        // decoded size = ISIZE, the payload's last four bytes (trailer of its only member; more
        // members -> RIO_ERR_UNSUPPORTED at decode). A member is at least 18 bytes, and above
        // DEFLATE's maximum ratio (258 bytes per 2 bits) no valid stream ends this way: the reader
        // fails on either.
        uint64_t isz = 0;
        if (plen >= 18) {
            const uint8_t* t = f + p + h.hdr_len + plen - 4;
            isz = t[0] | (uint64_t)t[1] << 8 | (uint64_t)t[2] << 16 | (uint64_t)t[3] << 24;
        }
        if (plen == 0 || plen < 18 || isz > 1032ull * plen + 64) {
            out_len = 0;
            pay = h.hdr_len;
            lflags = plen == 0 ? kEofBit : kBadBit;
            return RIO_OK;
        }
        out_len = isz;
    } else if (comp == RIO_COMP_LZW) {
        out_len = lzw_size(h.u, plen);
    } else {
        out_len = plen;
    }
    pay = ((plen - k) << 8) | (h.hdr_len + k);
    return RIO_OK;
}

// FileReader sequential semantics at record start p: header + payload availability + decoded
// size. next = start of the following record; pay = rec_pay descriptor (rio_device.h).
// Common records (canonical magic, header + preamble inside 32 bytes, valid) are parsed from two
// 16-byte loads; everything else (and every failure, for its exact classification) takes the
// byte-wise ReadUvarint restatement.
// A payload whose codec preamble / size already fails (snappy: unusable preamble; gzip: empty, too
// short, or an ISIZE no DEFLATE stream reaches) frames normally: FileReader consumed it, and its
// ReadNext fails without ending the file. `lflags` then carries kBadBit / kEofBit and out_len 0.
__device__ inline int frame_record(const uint8_t* f, uint64_t len, uint64_t p, uint32_t ver, uint32_t comp,
                            Hdr& h, uint64_t& next, uint64_t& out_len, uint64_t& pay, uint64_t& lflags,
                            const uint32_t* crct = nullptr) {
    lflags = 0;
    if (p + 32 <= len) {
        const uint4 a = ldu16(f + p), b = ldu16(f + p + 16);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (frame_fast(w, len, p, ver, comp, h, next, out_len, pay, crct) == RIO_OK) return RIO_OK;
    }
    return frame_slow(f, len, p, ver, comp, h, next, out_len, pay, lflags);
}

// ------------------------------------------------------------------------------------------
// File header (readFileHeaderFromBuffer, common_reader.go:22-44): every wave of the walks reads the 8
// header bytes itself (the per-call state reset, init_state, is the walks' own: rio_walk.hip)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int file_header_status(const FrameParams& P, uint32_t& v, uint32_t& c) {
    v = c = 0;
    if (P.len < RIO_FILE_HEADER_BYTES) return RIO_ERR_SHORT_FILE_HEADER;
    const uint8_t* f = P.file;
    v = f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    c = f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
    if (v > RIO_VERSION4 || v < RIO_VERSION1) return RIO_ERR_VERSION;
    if (c > RIO_COMP_LZW) return RIO_ERR_COMPRESSION_TYPE;
    return RIO_OK;
}

// ------------------------------------------------------------------------------------------
// Chunk bounds, magic candidates and the serial chunk walk
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t chunk_start(const FrameParams& P, uint64_t c) {
    return RIO_FILE_HEADER_BYTES + c * P.chunk_bytes;
}
__device__ __forceinline__ uint64_t chunk_end(const FrameParams& P, uint64_t c) {
    uint64_t e = chunk_start(P, c) + P.chunk_bytes;
    return e < P.len ? e : P.len;
}

// bytes 1 and 2 of a record's magic: 8d 4c (uvarint 0x130691, v2..v4), 06 13 (LE u32, v1)
__device__ __forceinline__ uint32_t magic3(uint32_t ver) { return ver == RIO_VERSION1 ? 0x130691u : 0x4C8D91u; }

// First position in [cs, ce) holding the canonical magic bytes 91 8d 4c (v1: 91 06 13) whose header
// and payload validate under FileReader semantics (CRC for v4). Speculative; stitched by the scan.
__device__ inline uint64_t find_entry(const FrameParams& P, uint64_t cs, uint64_t ce, uint32_t ver, uint32_t comp) {
    const uint8_t* f = P.file;
    const uint32_t m3 = magic3(ver);
    for (uint64_t q = cs & ~15ull; q < ce; q += 16) {
        const uint4 w = *reinterpret_cast<const uint4*>(f + q);
        uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = ws[k] ^ 0x91919191u;
            uint32_t hit = (x - 0x01010101u) & ~x & 0x80808080u;
            while (hit) {
                int b = __builtin_ctz(hit) >> 3;
                hit &= hit - 1;
                uint64_t p = q + 4 * k + b;
                if (p < cs || p >= ce || p + 2 >= P.len) continue;
                if (f[p + 1] != ((m3 >> 8) & 0xFF) || f[p + 2] != (m3 >> 16)) continue;
                Hdr h;
                uint64_t nx, ol, pd, lf;
                if (frame_record(f, P.len, p, ver, comp, h, nx, ol, pd, lf) == RIO_OK) return p;
            }
        }
    }
    return kNone;
}

// A walked record's slot as one 16-byte store / load (x, y = WalkSlot::len, z, w = WalkSlot::pos)
__device__ __forceinline__ void slot_store(WalkSlot* s, uint64_t rel, uint64_t len_flags, uint64_t pay) {
    const WalkSlot v = slot_pack(rel, len_flags, pay);
    *reinterpret_cast<uint4*>(s) =
        make_uint4((uint32_t)v.len, (uint32_t)(v.len >> 32), (uint32_t)v.pos, (uint32_t)(v.pos >> 32));
}
__device__ __forceinline__ WalkSlot slot_load(const WalkSlot* s) {
    const uint4 v = *reinterpret_cast<const uint4*>(s);
    return WalkSlot{(uint64_t)v.y << 32 | v.x, (uint64_t)v.w << 32 | v.z};
}

// Continue walking chunk c from record start p (count/bytes already in s), filling its scratch
// slots; sets s.exit / s.status. Serial header-to-header hops (FileReader order). p >= the chunk's start: a
// speculative entry lies in the chunk, and the repair enters a chunk where the chain left the one before it.
__device__ inline void walk_from(const FrameParams& P, uint64_t c, uint64_t p, uint32_t ver, uint32_t comp, ChunkSum& s,
                          const uint32_t* crct = nullptr) {
    const uint64_t cs = chunk_start(P, c), ce = chunk_end(P, c);
    WalkSlot* sc = P.scratch + c * P.slots;
    while (p < ce) {
        Hdr h;
        uint64_t next = 0, olen = 0, pd = 0, lf = 0;
        int e = frame_record(P.file, P.len, p, ver, comp, h, next, olen, pd, lf, crct);
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
        if (s.count < P.slots) slot_store(sc + s.count, p - cs, olen | lf | (h.nil ? kNilBit : 0), pd);
        s.count++;
        s.bytes += olen;
        p = next;
    }
    s.exit = s.status ? s.err_off : p;
}

__device__ __forceinline__ ChunkSum chunk_sum_empty(uint64_t entry) {
    ChunkSum s;
    s.entry = entry;
    s.exit = kNone;
    s.bytes = 0;
    s.err_off = 0;
    s.det0 = s.det1 = 0;
    s.count = 0;
    s.status = RIO_OK;
    return s;
}

// Walk chunk c from record start `from` (kNone => nothing to walk), filling its scratch slots.
__device__ inline void walk_chunk(const FrameParams& P, uint64_t c, uint64_t from, uint32_t ver, uint32_t comp) {
    ChunkSum s = chunk_sum_empty(from);
    if (from != kNone) walk_from(P, c, from, ver, comp, s);
    P.chunks[c] = s;
}

// exact per-byte equality with a byte value: bit 7 of every byte of the result = (byte == v)
__device__ __forceinline__ uint32_t bytes_eq(uint32_t d, uint32_t v4) {
    const uint32_t x = d ^ v4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// candidate bits of the 16 positions q .. q+15 in [lo, hi) (91 8d 4c at the position, the magic
// inside the file); d = the 16 bytes at q plus the next 4
__device__ __forceinline__ uint32_t magic_mask(const uint32_t (&d)[5], uint64_t q, uint64_t lo, uint64_t hi,
                                               uint64_t len, uint32_t m3) {
    // bytes equal to 0x91, gathered without a multiply: bit 8j + k of c = byte j of dword k (position
    // 4k + j); only those (~1 in 256 bytes) get the full 3-byte test and the bounds, in the loop
    // (round 4: the gather was a v_mul_lo_u32 per dword and the bounds a mask per block)
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) c |= bytes_eq(d[k], 0x91919191u) >> (7 - k);
    uint32_t mask = 0;
    if (c) {
        // positions [a, b) of the 16 are inside [lo, hi): lo and hi lie within 2^31 bytes of q (one
        // chunk's window, lo < hi), so 32-bit differences clamped to [0, 16] give a <= b; the three
        // magic bytes must lie in the file: i + 2 < len - q (64-bit: the file may extend far past q);
        // rio_ctx_create caps chunks at 1 GiB, which keeps lo and hi that close
        auto clamp16 = [](int32_t x) { return (uint32_t)(x < 0 ? 0 : (x > 16 ? 16 : x)); };
        const uint32_t a = clamp16((int32_t)((uint32_t)lo - (uint32_t)q));
        const uint32_t b = clamp16((int32_t)((uint32_t)hi - (uint32_t)q));
        const uint32_t lim = (uint32_t)umin(len - q, (uint64_t)18);
        do {
            const uint32_t bit = __ffs(c) - 1;
            c &= c - 1;
            const uint32_t k = bit & 7u, j = bit >> 3, i = 4 * k + j;
            const uint32_t d0 = k == 0 ? d[0] : (k == 1 ? d[1] : (k == 2 ? d[2] : d[3]));  // select, not index
            const uint32_t d1 = k == 0 ? d[1] : (k == 1 ? d[2] : (k == 2 ? d[3] : d[4]));
            const uint32_t x = __builtin_amdgcn_alignbyte(d1, d0, j) & 0xFFFFFFu;
            if (x == m3 && i >= a && i < b && i + 2 < lim) mask |= 1u << i;
        } while (c);
    }
    return mask;
}
}  // namespace rio
