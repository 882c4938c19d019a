// rio_seek.hip — single records and lookups on a file in HBM: MMapReader.ReadNextAt / SeekNext (k_read_at,
// k_seek_next), a batch of ReadNextAt offsets (k_readat_locate, k_readat_copy), the SeekNext map of a decoded file
// (k_count91 .. k_seek_jump) that serves the ReadAtI handle, and the DiskKeyIndex searches (k_index_search on the raw
// file, k_index_search_view on a decoded one). Framing primitives: rio_frame.h. Byte/integer work only; all offsets
// 64-bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_frame.h"
#include "rio_launch.h"
#include "rio_pb.h"
#include "rio_seg_copy.h"
#include "rio_wave.h"

namespace rio {

// ------------------------------------------------------------------------------------------
// Single record at an arbitrary offset: MMapReader.ReadNextAt (mmap_reader.go:130-203, 298-356)
// ------------------------------------------------------------------------------------------
// ReadNextAt up to the payload: bounds, header, nil, payload extent. RIO_OK with r.nil, or with
// r.payload_off / r.len (= the payload length in the file) set.
template <class B>
__device__ __forceinline__ int read_at_locate(B& get, uint64_t len, uint32_t ver, uint32_t comp, uint64_t off,
                                              ReadAtResult& r, Hdr& h, const uint32_t* crc_tab = nullptr) {
    r.nil = 0;
    r.len = 0;
    r.det0 = r.det1 = 0;
    if (off > len) return RIO_ERR_INVALID_OFFSET;  // x/exp/mmap ReadAt bounds
    // readNextAtV1 (mmap_reader.go:205-221): a 20-byte ReadAt short of its buffer fails wrapping io.EOF
    if (ver == RIO_VERSION1 && len - off < RIO_RECORD_HEADER_V1_BYTES) return RIO_EOF_HEADER;
    const uint64_t wmax = ver == RIO_VERSION4 ? RIO_RECORD_HEADER_V4_MAX : RIO_RECORD_HEADER_V3_MAX;
    const uint64_t w = len - off < wmax ? len - off : wmax;
    if (w == 0) return RIO_EOF;  // bare io.EOF
    int e = parse_header_t(get, off, w, ver == RIO_VERSION4 ? RIO_RECORD_HEADER_V4_MAX : ~0ull, ver, h, crc_tab);
    if (e == RIO_EOF) e = RIO_EOF_HEADER;
    if (e == RIO_ERR_HEADER_CRC) {
        r.det0 = h.exp_crc;
        r.det1 = h.act_crc;
    }
    if (e) return e;
    r.hdr_len = h.hdr_len;
    if (h.nil) {
        r.nil = 1;
        return RIO_OK;
    }
    const uint64_t plen = comp != RIO_COMP_NONE ? h.c : h.u;
    if (plen > len - off - h.hdr_len) return RIO_EOF_PAYLOAD;
    r.payload_off = off + h.hdr_len;
    r.len = plen;
    return RIO_OK;
}

__device__ int read_at_dev(const uint8_t* f, uint64_t len, uint32_t ver, uint32_t comp, uint64_t off,
                           uint8_t* out, uint64_t out_cap, ReadAtResult& r, bool write) {
    Hdr h;
    RawBytes raw{f};
    const int e0 = read_at_locate(raw, len, ver, comp, off, r, h);
    if (e0 || r.nil) return e0;
    const uint64_t plen = r.len;
    const uint8_t* pay = f + off + h.hdr_len;
    if (comp == RIO_COMP_NONE) {
        if (!write) return RIO_OK;
        if (plen > out_cap) return RIO_ERR_CAPACITY;
        for (uint64_t k = 0; k < plen; k++) out[k] = pay[k];
        return RIO_OK;
    }
    if (comp == RIO_COMP_GZIP || comp == RIO_COMP_LZW) {
        // gzip.NewReader on an empty payload: io.EOF (mmap_reader.go:189-191 wraps it); lzw: an empty
        // payload is io.ErrUnexpectedEOF. A payload to inflate / expand is the host's: it serves record
        // starts from the reader's decoded index and hands anything else back (r.payload_off / r.len
        // locate it)
        if (plen == 0) return comp == RIO_COMP_GZIP ? RIO_EOF_CODEC : RIO_ERR_DECOMPRESS;
        return RIO_ERR_UNSUPPORTED;
    }
    uint64_t dl = 0;
    const int k = uvarint_buf(pay, plen, dl);
    if (k <= 0 || dl > 0xFFFFFFFFull || dl > 22ull * (plen - (uint64_t)k) + 64) return RIO_ERR_DECOMPRESS;
    r.len = dl;
    if (dl > out_cap) return RIO_ERR_CAPACITY;
    if (!snappy_decode_thread(pay + k, plen - (uint64_t)k, out, dl)) return RIO_ERR_DECOMPRESS;
    return RIO_OK;
}

__global__ void k_read_at(const uint8_t* f, uint64_t len, uint64_t off, uint8_t* out, uint64_t out_cap,
                          ReadAtResult* res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ReadAtResult r{};
    uint32_t ver = 0, comp = 0;
    int e = RIO_OK;
    if (len < RIO_FILE_HEADER_BYTES) {
        e = RIO_ERR_SHORT_FILE_HEADER;
    } else {
        ver = f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
        comp = f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
        if (ver > RIO_VERSION4 || ver < RIO_VERSION1) e = RIO_ERR_VERSION;
        else if (comp > RIO_COMP_LZW) e = RIO_ERR_COMPRESSION_TYPE;
    }
    if (e == RIO_OK) e = read_at_dev(f, len, ver, comp, off, out, out_cap, r, true);
    r.status = e;
    *res = r;
}

// ------------------------------------------------------------------------------------------
// A batch of ReadNextAt queries on one file (rio_device_read_at_plan / _copy): what k_read_at answers for one offset,
// for n of them without a host synchronisation.
//   k_readat_locate     one lane per query: the file header as k_read_at reads it (a refused one is every hit's
//                       status), read_at_locate through the lane's 16-byte window, then the codec's part of
//                       read_at_dev up to the decode: the Snappy preamble and its bounds, gzip / lzw handed back
//                       located (RIO_ERR_UNSUPPORTED, payload_off / len) or failed on an empty payload. Writes the
//                       hit and the scan's input: the decoded length of an RIO_OK non-nil record, else 0
//   k_readat_copy<G>    first (the 16-lane launch only) the capacity rule, one lane per query: an RIO_OK non-nil
//                       hit whose range ends past out_cap becomes RIO_ERR_CAPACITY. Then, for an uncompressed file,
//                       copy_ranges (rio_seg_copy.h) from the file's payloads. The host does not know the file's
//                       compression (no synchronisation), so these and k_readat_snappy (rio_snappy.hip) are all
//                       launched and each reads the file header for itself
// The copy kernels trust no field of a hit: a range comes from out_off and is checked against out_cap by
// copy_ranges, a source from payload_off and is checked against the file.
// ------------------------------------------------------------------------------------------
namespace {
// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loop again
constexpr uint64_t kReadAtGridCap = 2048;

__device__ __forceinline__ int read_at_file_header(const uint8_t* f, uint64_t len, uint32_t& ver, uint32_t& comp) {
    FrameParams F{};
    F.file = f;
    F.len = len;
    return file_header_status(F, ver, comp);
}
}  // namespace

// position n holds the scan's last input, 0
__global__ void __launch_bounds__(256) k_readat_locate(ReadAtParams P) {
    // CRC-32C tables (T[0..255] = the byte table), copied here and not by crc32c_tab_init: a second caller changes that
    // function's out-of-line code, and k_index_search's registers are tuned around it as it is (rio_frame.h)
    __shared__ uint32_t T[1024];
    reinterpret_cast<uint4*>(T)[threadIdx.x] = reinterpret_cast<const uint4*>(kCrc32c.t)[threadIdx.x];  // 256 lanes
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t ver, comp;
    const int he = read_at_file_header(P.file, P.len, ver, comp);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= P.n; i += stride) {
        uint64_t need = 0;
        if (i < P.n) {
            ReadAtResult r{};
            int e = he;
            if (e == RIO_OK) {
                Hdr h;
                WinBytes wb{P.file};
                e = read_at_locate(wb, P.len, ver, comp, P.offsets[i], r, h, T);
                if (e == RIO_OK && !r.nil) {
                    if (comp == RIO_COMP_SNAPPY) {
                        uint32_t k;
                        uint64_t dl;
                        const bool ok = snappy_preamble_at(wb, r.payload_off, r.len, k, dl);
                        r.len = ok ? dl : 0;
                        if (!ok) e = RIO_ERR_DECOMPRESS;
                    } else if (comp != RIO_COMP_NONE) {
                        // read_at_dev's rule: an empty payload fails in the codec, any other is the host's to expand
                        e = r.len ? RIO_ERR_UNSUPPORTED : (comp == RIO_COMP_GZIP ? RIO_EOF_CODEC : RIO_ERR_DECOMPRESS);
                    }
                    if (e == RIO_OK) need = r.len;
                }
            }
            r.status = e;
            P.hits[i] = r;
        }
        P.tmp[i] = need;
    }
}

// G lanes per record. kLong = false: records shorter than kLongItem, and the capacity rule; true: the others.
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_readat_copy(ReadAtParams P) {
    if (!kLong) {
        // a hit marked here ends past out_cap, so no copy loop of this launch looks at it (copy_ranges skips the range
        // before it asks for a source); the launches after this one see the mark
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
            ReadAtResult& h = P.hits[i];
            if (h.status == RIO_OK && !h.nil && P.out_off[i + 1] > P.out_cap) h.status = RIO_ERR_CAPACITY;
        }
    }
    uint32_t ver, comp;
    if (read_at_file_header(P.file, P.len, ver, comp) != RIO_OK || comp != RIO_COMP_NONE) return;
    copy_ranges<G, kLong>(P.n, P.out_off, P.out_cap, P.out, [&](uint64_t j, uint64_t len) __attribute__((always_inline)) -> const uint8_t* {
        const ReadAtResult& h = P.hits[j];
        if (h.status != RIO_OK || h.nil || h.len != len || h.payload_off > P.len || len > P.len - h.payload_off)
            return nullptr;
        return P.file + h.payload_off;
    });
}

hipError_t launch_read_at_plan(const ReadAtParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_readat_locate, dim3(grid_for(P.n + 1, 256, kReadAtGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.out_off, P.n, s);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_read_at_copy(const ReadAtParams& P, hipStream_t s) {
    launch_short_long(k_readat_copy<16, false>, k_readat_copy<64, true>, P.n, P, s);
    return hipGetLastError();
}

// MMapReader.SeekNext (mmap_reader.go:58-128): windowed scan for 91 8d 4c with its skip rule,
// trial ReadNextAt per hit; CRC / magic / io.EOF-class failures continue the scan. Returns the
// status; on RIO_OK r describes the record at rec_off (payload_off / len when !write).
template <class B, class Trial>
__device__ __forceinline__ int seek_next_t(B& get, uint64_t len, uint64_t off, uint64_t seek_len, Trial&& trial, uint64_t& rec_off) {
    const uint8_t M[3] = {0x91, 0x8D, 0x4C};
    rec_off = 0;
    uint64_t next = off;
    for (;;) {
        if (next > len) return RIO_ERR_INVALID_OFFSET;
        const uint64_t num = len - next < seek_len ? len - next : seek_len;
        if (num == 0) return RIO_EOF;
        uint64_t i = 0;
        bool boundary = false;
        while (i < num) {
            uint64_t ix = i;
            for (int j = 0; j < 3; j++) {
                if (get(next + ix) != M[j]) break;
                ix++;
                if (ix >= num) {
                    boundary = true;
                    break;
                }
            }
            if (boundary) break;
            if (ix - i < 3) {
                i = ix + 1;
                continue;
            }
            const uint64_t at = next + i;
            const int te = trial(at);
            if (te != RIO_OK && (te == RIO_ERR_HEADER_CRC || te == RIO_ERR_MAGIC || te == RIO_EOF ||
                                 te == RIO_EOF_HEADER || te == RIO_EOF_PAYLOAD || te == RIO_EOF_CODEC)) {
                i = ix;
                continue;
            }
            rec_off = at;
            return te;
        }
        if (i == 0) return RIO_EOF;
        next += i;
    }
}

__device__ int seek_next_dev(const uint8_t* f, uint64_t len, uint32_t ver, uint32_t comp, uint64_t off,
                             uint64_t seek_len, uint8_t* out, uint64_t out_cap, bool write, ReadAtResult& r,
                             uint64_t& rec_off) {
    RawBytes raw{f};
    return seek_next_t(raw, len, off, seek_len,
                       [&](uint64_t at) { return read_at_dev(f, len, ver, comp, at, out, out_cap, r, write); }, rec_off);
}

__device__ __forceinline__ int file_header_dev(const uint8_t* f, uint64_t len, uint32_t& ver, uint32_t& comp) {
    ver = comp = 0;
    if (len < RIO_FILE_HEADER_BYTES) return RIO_ERR_SHORT_FILE_HEADER;
    ver = f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    comp = f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
    if (ver > RIO_VERSION4 || ver < RIO_VERSION1) return RIO_ERR_VERSION;
    if (comp > RIO_COMP_LZW) return RIO_ERR_COMPRESSION_TYPE;
    if (ver < RIO_VERSION2) return RIO_ERR_UNSUPPORTED;  // SeekNext: mmap_reader.go:62-64
    return RIO_OK;
}

__global__ void k_seek_next(const uint8_t* f, uint64_t len, uint64_t off, uint64_t seek_len, uint8_t* out,
                            uint64_t out_cap, ReadAtResult* res, uint64_t* rec_off) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ReadAtResult r{};
    uint64_t ro = 0;
    uint32_t ver, comp;
    int e = file_header_dev(f, len, ver, comp);
    if (e == RIO_OK) e = seek_next_dev(f, len, ver, comp, off, seek_len, out, out_cap, true, r, ro);
    r.status = e;
    *rec_off = ro;
    *res = r;
}

// ------------------------------------------------------------------------------------------
// SeekNext map of a decoded file (rio_reader_seek_next). MMapReader.SeekNext (mmap_reader.go:58-128)
// visits positions from its offset one by one; only a 0x91 byte changes the walk: 91 X (X != 8d)
// jumps to p+2, 91 8d Y (Y != 4c) to p+3, and a marker 91 8d 4c runs a trial ReadNextAt whose
// io.EOF / magic / header-CRC class continues at p+3 while anything else ends the call. With windows
// of >= 4 bytes the walk does not depend on where windows start (a marker cut by a window end is
// re-read from its start). So the answer from offset s is fixed by the first 0x91 at or after s:
// P = every 0x91 position in file order, R[k] = the walk's end from P[k] — a record j of the decoded
// sequence (its trial is record j, answered from the decoded arena), kSeekEof (the walk passes the
// last 0x91 and the scan reads to the file end: io.EOF) or kSeekOther (a trial outside the sequence
// that ends the walk: the single-record kernel answers those; a partial marker at the file end is
// kSeekEof, as the reference's rewind there returns io.EOF). Built once per reader:
//   k_count91 / k_scan_segs / k_list91: P (a wave per 4 KiB segment, ballot-free lane prefix);
//   k_seek_step: each position's own step (terminal, or the index of the next 0x91 visited);
//   k_seek_jump: pointer jumping to each walk's end (log2 of the longest walk rounds).
// ------------------------------------------------------------------------------------------
constexpr uint64_t kSeekOther = RIO_SEEK_END_OTHER;  // rio.h: rio_reader_index_info shows R as it is
constexpr uint64_t kSeekEof = RIO_SEEK_END_EOF;  // the walk passed the last 0x91 without a trial ending it: io.EOF
constexpr uint64_t kSeekTerm = 1ull << 63;
constexpr uint32_t kSegBytes = 4096;

__device__ __forceinline__ uint32_t count91(const uint8_t* f, uint64_t at, uint64_t len, uint32_t* mask4) {
    // bytes [at, at + 64) equal to 0x91 (bounded by len); mask4[q]: bit j = byte 16q + j. Loads stay
    // below len + RIO_DEVICE_PAD: a lane starting at or past len reads nothing
    uint32_t c = 0;
    if (at >= len) {
        mask4[0] = mask4[1] = mask4[2] = mask4[3] = 0;
        return 0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = *reinterpret_cast<const uint4*>(f + at + 16 * q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                m |= (((w[t] >> (8 * j)) & 0xFFu) == 0x91u ? 1u : 0u) << (4 * t + j);
        const uint64_t base = at + 16 * q;
        if (base + 16 > len) m &= base >= len ? 0u : ((1u << (len - base)) - 1u);
        mask4[q] = m;
        c += __builtin_popcount(m);
    }
    return c;
}

__global__ void __launch_bounds__(256) k_count91(const uint8_t* f, uint64_t len, uint64_t nseg, uint64_t* cnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    uint32_t m[4];
    const uint32_t c = count91(f, seg * kSegBytes + lane * 64, len, m);
    uint32_t total;
    (void)wave_excl(c, lane, total);
    if (lane == 0) cnt[seg] = total;
}

// exclusive prefix sum of cnt[0, n) in place, one block; cnt[n] = the total
__global__ void __launch_bounds__(1024) k_scan_segs(uint64_t* cnt, uint64_t n) {
    __shared__ uint64_t part[1024];
    const uint64_t per = (n + 1023) / 1024, a = threadIdx.x * per, b = a + per < n ? a + per : n;
    uint64_t sum = 0;
    for (uint64_t i = a; i < b; i++) sum += cnt[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - sum;
    for (uint64_t i = a; i < b; i++) {
        const uint64_t c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    if (threadIdx.x == 1023) cnt[n] = part[1023];
}

__global__ void __launch_bounds__(256) k_list91(const uint8_t* f, uint64_t len, uint64_t nseg, const uint64_t* base,
                                                uint64_t* P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const uint64_t at = seg * kSegBytes + lane * 64;
    uint32_t m[4];
    const uint32_t c = count91(f, at, len, m);
    uint32_t total;
    uint64_t o = base[seg] + wave_excl(c, lane, total);
    for (int q = 0; q < 4; q++)
        for (uint32_t x = m[q]; x; x &= x - 1) P[o++] = at + 16 * q + __builtin_ctz(x);
}

__device__ __forceinline__ uint64_t lower_u64(const uint64_t* a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_seek_step(const uint8_t* f, uint64_t len, const uint64_t* P, uint64_t K,
                                                   const uint64_t* rec_off, const uint8_t* flags, uint64_t n,
                                                   uint64_t* step) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t ver = 0, comp = 0;
    const int he = file_header_dev(f, len, ver, comp);
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const uint64_t p = P[k];
        uint64_t out = kSeekTerm | kSeekOther, c = 0;
        if (he == RIO_OK && (p + 1 >= len || (f[p + 1] == 0x8D && p + 2 >= len))) {
            // a partial marker at the file end: SeekNext re-reads from it, its window ends inside the
            // marker with i == 0, and the call returns io.EOF (mmap_reader.go:88-124)
            out = kSeekTerm | kSeekEof;
        } else if (he == RIO_OK) {
            if (f[p + 1] != 0x8D) {
                c = p + 2;
            } else {
                if (f[p + 2] != 0x4C) {
                    c = p + 3;
                } else {
                    const uint64_t j = lower_u64(rec_off, n, p);
                    if (j < n && rec_off[j] == p) {
                        if (flags[j] & RIO_FLAG_EOF) c = p + 3;  // its trial is io.EOF class: the walk goes on
                        else out = kSeekTerm | j;
                    } else {  // a marker outside the decoded sequence: its own trial, as the reference runs it
                        ReadAtResult r{};
                        Hdr h;
                        RawBytes raw{f};
                        const int te = read_at_locate(raw, len, ver, comp, p, r, h);
                        const bool benign = te == RIO_ERR_HEADER_CRC || te == RIO_ERR_MAGIC || te == RIO_EOF ||
                                            te == RIO_EOF_HEADER || te == RIO_EOF_PAYLOAD ||
                                            (te == RIO_OK && !r.nil && comp == RIO_COMP_GZIP && r.len == 0);
                        if (benign) c = p + 3;
                    }
                }
            }
        }
        if (c) {
            const uint64_t nk = lower_u64(P, K, c);
            out = nk < K ? nk : (kSeekTerm | kSeekEof);  // no 0x91 left: the scan reads to the file end
        }
        step[k] = out;
    }
}

__global__ void __launch_bounds__(256) k_seek_jump(const uint64_t* in, uint64_t* out, uint64_t K) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const uint64_t v = in[k];
        out[k] = (v & kSeekTerm) ? v : in[v];
    }
}

// P and R (host vectors) of a device-resident file and its decoded record offsets / flags
int build_seek_map(const uint8_t* f, uint64_t len, const uint64_t* rec_off, const uint8_t* flags, uint64_t n,
                   std::vector<uint64_t>& P, std::vector<uint64_t>& R, hipStream_t s) {
    P.clear();
    R.clear();
    const uint64_t nseg = (len + kSegBytes - 1) / kSegBytes;
    if (nseg == 0) return 0;
    uint64_t *cnt = nullptr, *dP = nullptr, *a = nullptr, *b = nullptr;
    auto done = [&](int rc) {
        if (cnt) (void)hipFree(cnt);
        if (dP) (void)hipFree(dP);
        if (a) (void)hipFree(a);
        if (b) (void)hipFree(b);
        return rc;
    };
    if (hipMalloc(&cnt, (nseg + 1) * 8) != hipSuccess) return done(-1);
    const unsigned gs = (unsigned)((nseg + 3) / 4);
    hipLaunchKernelGGL(k_count91, dim3(gs), dim3(256), 0, s, f, len, nseg, cnt);
    hipLaunchKernelGGL(k_scan_segs, dim3(1), dim3(1024), 0, s, cnt, nseg);
    uint64_t K = 0;
    if (hipMemcpyAsync(&K, cnt + nseg, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(-1);
    if (K == 0) return done(0);
    if (hipMalloc(&dP, K * 8) != hipSuccess || hipMalloc(&a, K * 8) != hipSuccess || hipMalloc(&b, K * 8) != hipSuccess)
        return done(-1);
    hipLaunchKernelGGL(k_list91, dim3(gs), dim3(256), 0, s, f, len, nseg, cnt, dP);
    hipLaunchKernelGGL(k_seek_step, dim3(1024), dim3(256), 0, s, f, len, dP, K, rec_off, flags, n, a);
    for (int round = 0; round < 40; round++) {  // walks of up to 2^40 steps
        hipLaunchKernelGGL(k_seek_jump, dim3(1024), dim3(256), 0, s, a, b, K);
        std::swap(a, b);
    }
    P.resize(K);
    R.resize(K);
    if (hipMemcpyAsync(P.data(), dP, K * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(R.data(), a, K * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(-1);
    for (uint64_t& r : R) r = (r & kSeekTerm) ? (r & ~kSeekTerm) : kSeekOther;  // unfinished walks: the kernel
    return done(hipGetLastError() == hipSuccess ? 0 : -1);
}

// ------------------------------------------------------------------------------------------
// DiskKeyIndex lookups (sstables/disk_key_index.go:87-140), one lane per query key: the reference's
// binarySearch over byte offsets [0, size) of an uncompressed index.rio, each probe findAt(h) =
// SeekNext(h) + proto.Unmarshal into an IndexEntry, compared with bytes.Compare. Every lane runs
// the exact probe sequence of a freshly loaded index (SeekNext is not monotone in h because of the
// scan's skip rule, so a table of record starts alone would not reproduce it).
// ------------------------------------------------------------------------------------------
// bytes.Compare(file[a, a + an), key[0, bn)): the file side through the lane's window
__device__ __forceinline__ int bytes_compare_dev(WinBytes& wb, uint64_t a, uint64_t an, const uint8_t* b, uint64_t bn) {
    const uint64_t m = an < bn ? an : bn;
    for (uint64_t k = 0; k < m; k++) {
        const uint32_t x = wb(a + k), y = b[k];
        if (x != y) return x < y ? -1 : 1;
    }
    return an < bn ? -1 : (an > bn ? 1 : 0);
}

// findAt: 0 and the entry's fields (key_off absolute in f), or a status. All bytes come through the
// lane's 16-byte window: one load per 16 bytes scanned or parsed instead of one per byte (the
// kernel is bound by L2 requests, not by latency).
__device__ __forceinline__ int index_find_at(WinBytes& wb, uint64_t len, uint32_t ver, uint64_t h, uint64_t seek_len,
                                             const uint32_t* T, uint64_t& ko, uint64_t& kl, uint64_t& vo, uint64_t& cs) {
    ReadAtResult r{};
    Hdr hd;
    uint64_t ro;
    const int e = seek_next_t(
        wb, len, h, seek_len,
        [&](uint64_t at) __attribute__((always_inline)) {
            return read_at_locate(wb, len, ver, RIO_COMP_NONE, at, r, hd, T);
        },
        ro);
    if (e) return e;
    const uint64_t pl = r.nil ? 0 : r.len;
    const uint64_t po = r.nil ? 0 : r.payload_off;
    if (!pb_index_entry_t(wb, po, pl, ko, kl, vo, cs)) return RIO_ERR_PROTO;
    ko += po;
    return RIO_OK;
}

__device__ __forceinline__ bool eof_class(int e) {
    return e == RIO_EOF || e == RIO_EOF_ZERO_TAIL || e == RIO_EOF_HEADER || e == RIO_EOF_PAYLOAD || e == RIO_EOF_CODEC;
}

// minimum waves per SIMD for k_index_search (0 = the compiler's choice: 129 VGPRs, 3 waves). Measured on
// the idx bench (M lookups/s): 3 waves 155.6, 4 189.3, 5 199.0, 6 21.2 (3393 scratch ops in the probe
// loop), 8 228.9 (64 VGPRs, 384 B scratch, 281 scratch ops). The spill placement is the compiler's and
// changes with the bound; re-measure after touching this kernel.
constexpr uint32_t kIdxOcc = 8;
__global__ void __launch_bounds__(256, kIdxOcc) k_index_search(
    const uint8_t* f, uint64_t len, uint64_t seek_len, const uint8_t* keys, const uint64_t* key_off, uint64_t nq,
    const uint32_t* perm, rio_index_hit* hits) {
    __shared__ uint32_t T[1024];  // CRC-32C tables (T[0..255] = the byte table)
    crc32c_tab_init(T);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t ver, comp;
    const int he = file_header_dev(f, len, ver, comp);
    for (uint64_t qq = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; qq < nq; qq += stride) {
        const uint64_t q = perm ? perm[qq] : qq;  // queries in key order (rio_sort.hip), results in place
        rio_index_hit out{};
        const uint8_t* key = keys + key_off[q];
        const uint64_t klen = key_off[q + 1] - key_off[q];
        int e = he;
        if (e == RIO_OK && comp != RIO_COMP_NONE) e = RIO_ERR_UNSUPPORTED;
        uint64_t ko = 0, kl = 0, vo = 0, cs = 0;
        WinBytes wb{f};
        if (e == RIO_OK) {
            uint64_t i = 0, j = len;
            while (i < j) {
                const uint64_t h = (i + j) >> 1;
                e = index_find_at(wb, len, ver, h, seek_len, T, ko, kl, vo, cs);
                if (e) break;
                if (bytes_compare_dev(wb, ko, kl, key, klen) < 0) i = h + 1; else j = h;
            }
            if (e == RIO_OK) {
                e = index_find_at(wb, len, ver, i, seek_len, T, ko, kl, vo, cs);
                if (e == RIO_OK) {
                    out.offset = i;
                    out.found = i < len && bytes_compare_dev(wb, ko, kl, key, klen) == 0;
                    if (out.found) {
                        out.value_offset = vo;
                        out.checksum = cs;
                    }
                }
            }
            if (eof_class(e)) {  // binarySearch: an io.EOF probe means "not found" at offset size
                e = RIO_OK;
                out.offset = len;
            }
        }
        out.status = e;
        hits[q] = out;
    }
}

// DiskKeyIndex lookups on a compressed index.rio (rio_index_open builds the view): the same binarySearch
// per query lane, each probe findAt(h) answered from the decoded records and the SeekNext map instead
// of the raw file: the first 0x91 at or after h fixes SeekNext's answer (windows of 4096 bytes), which
// is record R[k] (its IndexEntry parsed from the decoded arena), io.EOF (no 0x91 left, or a walk that
// runs past the last one), the record's codec error, or a trial outside the decoded sequence (handed
// back: RIO_ERR_UNSUPPORTED for that query).
__device__ __forceinline__ int index_view_find_at(const uint8_t* out, const uint64_t* out_off, const uint8_t* flags,
                                                  uint64_t n, const uint64_t* P, uint64_t K, const uint64_t* R,
                                                  uint64_t h, uint64_t& ko, uint64_t& kl, uint64_t& vo, uint64_t& cs) {
    const uint64_t k = lower_u64(P, K, h);
    if (k >= K) return RIO_EOF;
    const uint64_t r = R[k];
    if (r == kSeekEof) return RIO_EOF;
    if (r >= n) return RIO_ERR_UNSUPPORTED;
    if (flags[r] & RIO_FLAG_CORRUPT) return RIO_ERR_DECOMPRESS;
    if (flags[r] & RIO_FLAG_EOF) return RIO_EOF_CODEC;  // (the map walks past those)
    const uint64_t base = out_off[r], pl = out_off[r + 1] - base;  // a nil record: no bytes
    if (!pb_index_entry(out + base, pl, ko, kl, vo, cs)) return RIO_ERR_PROTO;
    ko += base;
    return RIO_OK;
}

__device__ __forceinline__ int bytes_compare_mem(const uint8_t* a, uint64_t an, const uint8_t* b, uint64_t bn) {
    const uint64_t m = an < bn ? an : bn;
    for (uint64_t k = 0; k < m; k++)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return an < bn ? -1 : (an > bn ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_index_search_view(const uint8_t* out, const uint64_t* out_off,
                                                           const uint8_t* flags, uint64_t n, const uint64_t* P,
                                                           uint64_t K, const uint64_t* R, uint64_t len,
                                                           const uint8_t* keys, const uint64_t* key_off, uint64_t nq,
                                                           const uint32_t* perm, rio_index_hit* hits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t qq = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; qq < nq; qq += stride) {
        const uint64_t q = perm ? perm[qq] : qq;
        rio_index_hit o{};
        const uint8_t* key = keys + key_off[q];
        const uint64_t klen = key_off[q + 1] - key_off[q];
        uint64_t ko = 0, kl = 0, vo = 0, cs = 0, i = 0, j = len;
        int e = RIO_OK;
        while (i < j) {
            const uint64_t h = (i + j) >> 1;
            e = index_view_find_at(out, out_off, flags, n, P, K, R, h, ko, kl, vo, cs);
            if (e) break;
            if (bytes_compare_mem(out + ko, kl, key, klen) < 0) i = h + 1; else j = h;
        }
        if (e == RIO_OK) {
            e = index_view_find_at(out, out_off, flags, n, P, K, R, i, ko, kl, vo, cs);
            if (e == RIO_OK) {
                o.offset = i;
                o.found = i < len && bytes_compare_mem(out + ko, kl, key, klen) == 0;
                if (o.found) {
                    o.value_offset = vo;
                    o.checksum = cs;
                }
            }
        }
        if (eof_class(e)) {  // binarySearch: an io.EOF probe means "not found" at offset size
            e = RIO_OK;
            o.offset = len;
        }
        o.status = e;
        hits[q] = o;
    }
}

hipError_t launch_index_search_view(const uint8_t* out, const uint64_t* out_off, const uint8_t* flags, uint64_t n,
                                    const uint64_t* P, uint64_t K, const uint64_t* R, uint64_t len, const uint8_t* keys,
                                    const uint64_t* key_off, uint64_t nq, const uint32_t* perm, rio_index_hit* hits,
                                    hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint64_t blocks = (nq + 255) / 256;
    hipLaunchKernelGGL(k_index_search_view, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, out,
                       out_off, flags, n, P, K, R, len, keys, key_off, nq, perm, hits);
    return hipGetLastError();
}

hipError_t launch_read_at(const uint8_t* f, uint64_t len, uint64_t off, uint8_t* out, uint64_t out_cap,
                          ReadAtResult* res, hipStream_t s) {
    hipLaunchKernelGGL(k_read_at, dim3(1), dim3(64), 0, s, f, len, off, out, out_cap, res);
    return hipGetLastError();
}

hipError_t launch_seek_next(const uint8_t* f, uint64_t len, uint64_t off, uint64_t seek_len, uint8_t* out,
                            uint64_t out_cap, ReadAtResult* res, uint64_t* rec_off, hipStream_t s) {
    hipLaunchKernelGGL(k_seek_next, dim3(1), dim3(64), 0, s, f, len, off, seek_len, out, out_cap, res, rec_off);
    return hipGetLastError();
}

hipError_t launch_index_search(const uint8_t* f, uint64_t len, uint64_t seek_len, const uint8_t* keys,
                               const uint64_t* key_off, uint64_t nq, const uint32_t* perm, rio_index_hit* hits,
                               hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint64_t blocks = (nq + 255) / 256;
    hipLaunchKernelGGL(k_index_search, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, f, len,
                       seek_len, keys, key_off, nq, perm, hits);
    return hipGetLastError();
}
}  // namespace rio
