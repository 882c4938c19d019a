// rio_flush.hip — flush of a memstore on the device: MemStore.Flush / FlushWithTombstones
// (memstore/memstore.go:189-238) for a memstore kept as an append-only log of operations. The reference
// keeps a skip list ordered by key and walks it at flush; here nothing is ordered until the flush, which
// sorts the log by (key, op index), keeps the last op of every key and hands "source order + keep flags +
// one view" to the compaction back end (rio_sst_merge_gather, rio_device_encode, rio_sst_index_encode).
//
// Order: bytes.Compare on the key (lexicographic, unsigned, a proper prefix first), then the op index.
// LSD radix sort over 64-bit digits with stable passes (hipcub::DeviceRadixSort::SortPairs of (digit, op)):
// with R = ceil(max_key_len / 8), the least significant digit is the key length, then come the key's
// 8-byte chunks R-1 .. 0 read big-endian and zero-padded past the key's end. Two keys that differ at some
// byte differ in that byte's chunk and every more significant chunk is equal; a key that is a proper
// prefix of another (trailing zero bytes included: "a" / "a\0") has equal padded chunks and the smaller
// length. The first permutation is the identity and every pass is stable, so equal keys stay in op
// order. R + 1 passes, no segment bookkeeping, no host round trip, work linear in the log whatever prefixes
// the keys share.
//
//   k_flush_check  one lane per op: key and value ranges monotone and inside their arenas, key length
//                  <= max_key_len (first offending op -> RIO_MERGE_R_UNSORTED); writes the clamped key
//                  length, the identity permutation and the length digit
//   k_flush_digit  one lane per position of the order so far: that op's chunk c as a big-endian word (the
//                  last chunk shifted down to its used bytes); one unaligned 8-byte load, masked at the
//                  key's end (it may pass the key's end by up to 7 bytes: inside the arena or its
//                  RIO_DEVICE_PAD)
//   k_flush_keep   one lane per sorted position: kept when the next position holds another key (lengths,
//                  then the bytes) or there is none, and, under RIO_FLUSH_SKIP_TOMBSTONES, when the op is
//                  not nil (an empty non-nil value is kept, memstore.go:229); source word, keep flag, the
//                  result block's sums
//   k_flush_crc    one lane per kept position: CRC-64/ISO of the op's value (rio_crc64.h, the code of
//                  k_sst_validate) into crc[op], which the index encode reads through the registered view
// Every op index read back from a buffer is clamped to [0, n), every range to its arena: a wrong input
// gives a status or wrong bytes, never an out-of-range access.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "rio_crc64.h"
#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_ops_keys.h"

namespace rio {

namespace {

// 256 CUs x 8 blocks of 256 lanes: longer logs go round the grid-stride loops again
constexpr uint64_t kFlushGridCap = 2048;

typedef uint64_t __attribute__((aligned(1))) u64u;

// key of a checked op: the offset clamped again, the length k_flush_check left (at most max_key_len and
// inside the arena from that offset on)
__device__ __forceinline__ const uint8_t* key_of(const FlushParams& P, uint64_t op, uint64_t& len) {
    const uint64_t off = umin(P.ops.key_off[op], P.ops.key_bytes);
    len = umin(P.key_len[op], P.ops.key_bytes - off);
    return P.ops.keys + off;
}
// bytes [8c, 8c + 8) of a key as a big-endian word, zero from the key's end on
__device__ __forceinline__ uint64_t key_chunk(const uint8_t* k, uint64_t len, uint64_t c) {
    const uint64_t b = 8 * c;
    if (b >= len) return 0;
    uint64_t w = __builtin_bswap64(*reinterpret_cast<const u64u*>(k + b));
    const uint64_t m = len - b;
    if (m < 8) w &= ~0ull << (8 * (8 - m));
    return w;
}
__device__ __forceinline__ uint64_t op_at(const uint32_t* perm, uint64_t p, uint64_t n) {
    const uint64_t op = perm[p];
    return op < n ? op : 0;
}

}  // namespace

__global__ void k_flush_init(uint64_t* r) {
    if (threadIdx.x < RIO_MERGE_RESULT_WORDS)
        r[threadIdx.x] = (threadIdx.x == RIO_MERGE_R_FIRST_DUP || threadIdx.x == RIO_MERGE_R_UNSORTED) ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(256) k_flush_check(FlushParams P) {
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(&P.result[RIO_MERGE_R_UNSORTED]);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.ops.n; i += stride) {
        uint64_t off, len, vb, ve;
        const bool ok = key_range(P.ops, P.max_key_len, i, off, len);
        const bool okv = value_range(P.ops, i, vb, ve);
        P.key_len[i] = len;
        P.perm[0][i] = (uint32_t)i;
        P.dig[0][i] = len;
        if (!(ok && okv)) atomicMin(bad, (unsigned long long)i);
    }
}

__global__ void __launch_bounds__(256) k_flush_digit(FlushParams P, const uint32_t* perm, uint64_t chunk,
                                                     uint32_t shift) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P.ops.n; p += stride) {
        uint64_t len;
        const uint8_t* k = key_of(P, op_at(perm, p, P.ops.n), len);
        P.dig[0][p] = key_chunk(k, len, chunk) >> shift;
    }
}

__global__ void __launch_bounds__(256) k_flush_keep(FlushParams P, const uint32_t* perm) {
    unsigned long long* R = reinterpret_cast<unsigned long long*>(P.result);
    const uint64_t n = P.ops.n, stride = (uint64_t)gridDim.x * blockDim.x;
    // the result block's sums: LDS atomics per round, then one global atomic per block, round and sum
    // (whole blocks iterate together for the barriers)
    __shared__ unsigned long long s_sum[4];
    const uint64_t rounds = (n + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t p = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
        __syncthreads();
        if (p < n) {
            const uint64_t op = op_at(perm, p, n);
            uint64_t len;
            const uint8_t* k = key_of(P, op, len);
            bool last = p + 1 == n;
            if (!last) {
                uint64_t nlen;
                const uint8_t* nk = key_of(P, op_at(perm, p + 1, n), nlen);
                last = nlen != len;
                for (uint64_t c = 0; !last && 8 * c < len; c++) last = key_chunk(k, len, c) != key_chunk(nk, len, c);
            }
            uint64_t vb, ve;
            value_range(P.ops, op, vb, ve);
            const bool nil = (P.ops.flags[op] & RIO_FLAG_NIL) != 0;
            const uint64_t vlen = nil ? 0 : ve - vb;
            const bool keep = last && !(nil && P.mode == RIO_FLUSH_SKIP_TOMBSTONES);
            P.src[p] = op;
            P.keep[p] = keep ? 1 : 0;
            if (keep) {
                atomicAdd(&s_sum[0], 1ull);
                if (vlen) atomicAdd(&s_sum[1], (unsigned long long)vlen);
                if (nil) atomicAdd(&s_sum[2], 1ull);
                if (len) atomicAdd(&s_sum[3], (unsigned long long)len);
            }
        }
        __syncthreads();
        if (threadIdx.x < 4 && s_sum[threadIdx.x]) {
            const uint32_t word = threadIdx.x == 0 ? RIO_MERGE_R_N_OUT : threadIdx.x == 1 ? RIO_MERGE_R_VALUE_BYTES
                                : threadIdx.x == 2 ? RIO_MERGE_R_NULL_VALUES : RIO_MERGE_R_KEY_BYTES;
            atomicAdd(&R[word], s_sum[threadIdx.x]);
        }
    }
}

__global__ void __launch_bounds__(256) k_flush_crc(FlushParams P) {
    __shared__ uint64_t tab[8][256];  // 16 KiB
    crc64_build_table(tab);
    const uint64_t n = P.ops.n, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (!P.keep[p]) continue;
        const uint64_t w = P.src[p], op = w < n ? w : 0;
        uint64_t vb, ve;
        value_range(P.ops, op, vb, ve);
        const bool nil = (P.ops.flags[op] & RIO_FLAG_NIL) != 0;
        P.crc[op] = crc64_value(tab, P.ops.values + vb, nil ? 0 : ve - vb);  // a nil value hashes as empty
    }
}

namespace {

struct PassBits {
    int begin, end;
};
// chunk passes sort all 64 bits, except the last chunk (the first pass after the length): keys end at
// max_key_len, so its low bytes are zero in every digit. Those digits are shifted down by chunk_shift and
// sorted over the bits that are left, from bit 0: every pass's bit range starts at 0 (rocPRIM's merge path,
// taken for some 10^3 .. 10^6 items, builds its compare mask as (1 << end_bit) - 1, which is wrong for a range
// that ends at bit 64 and starts above 0)
uint32_t chunk_shift(uint32_t max_key_len, uint32_t chunk) {
    const uint32_t R = (max_key_len + 7) / 8;
    return chunk + 1 != R ? 0 : 64 - 8 * (max_key_len - 8 * chunk);
}
PassBits chunk_bits(uint32_t max_key_len, uint32_t chunk) { return {0, (int)(64 - chunk_shift(max_key_len, chunk))}; }
PassBits length_bits(uint32_t max_key_len) {
    int b = 1;
    while ((max_key_len >> b) != 0) b++;
    return {0, b};
}

size_t sort_bytes(uint64_t n, PassBits b) {
    size_t t = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, b.begin, b.end) !=
        hipSuccess)
        return 0;
    return t;
}

}  // namespace

size_t flush_cub_bytes(uint64_t n, uint32_t max_key_len) {
    const uint32_t R = (max_key_len + 7) / 8;
    size_t t = sort_bytes(n, length_bits(max_key_len));
    if (R) t = std::max(t, sort_bytes(n, chunk_bits(max_key_len, R - 1)));
    if (R > 1) t = std::max(t, sort_bytes(n, PassBits{0, 64}));
    return t;
}

// ev (timing on): kFlushMaxStages + 1 events; ev[k] .. ev[k + 1] bracket stage k (check, the length pass,
// the chunk passes R-1 .. 0, keep, crc); *n_stages = stages recorded. with_crc = false leaves the crc stage out
// (rio_mem_index_build: nothing reads the values' checksums)
hipError_t launch_flush_plan(const FlushParams& P, hipStream_t s, hipEvent_t* ev, uint32_t* n_stages, bool with_crc) {
    uint32_t k = 0;
    auto stamp = [&]() {
        if (ev) hipEventRecord(ev[k], s);
        k++;
    };
    const uint64_t n = P.ops.n;
    hipLaunchKernelGGL(k_flush_init, dim3(1), dim3(64), 0, s, P.result);
    *n_stages = 0;
    if (!n) return hipGetLastError();
    const dim3 g(grid_for(n, 256, kFlushGridCap)), b(256);
    stamp();
    hipLaunchKernelGGL(k_flush_check, g, b, 0, s, P);
    stamp();
    uint32_t cur = 0;  // P.perm[cur] holds the order so far
    auto sort = [&](PassBits bits) {
        size_t tb = P.cub_bytes;
        const hipError_t e = hipcub::DeviceRadixSort::SortPairs(P.cub, tb, (const uint64_t*)P.dig[0], P.dig[1],
                                                                (const uint32_t*)P.perm[cur], P.perm[cur ^ 1], (int)n,
                                                                bits.begin, bits.end, s);
        cur ^= 1;
        return e;
    };
    hipError_t e = sort(length_bits(P.max_key_len));
    if (e != hipSuccess) return e;
    stamp();
    for (uint32_t c = (P.max_key_len + 7) / 8; c-- > 0;) {
        hipLaunchKernelGGL(k_flush_digit, g, b, 0, s, P, (const uint32_t*)P.perm[cur], (uint64_t)c,
                           chunk_shift(P.max_key_len, c));
        e = sort(chunk_bits(P.max_key_len, c));
        if (e != hipSuccess) return e;
        stamp();
    }
    hipLaunchKernelGGL(k_flush_keep, g, b, 0, s, P, (const uint32_t*)P.perm[cur]);
    stamp();
    if (with_crc) {
        hipLaunchKernelGGL(k_flush_crc, g, b, 0, s, P);
        stamp();
    }
    *n_stages = k - 1;
    return hipGetLastError();
}

}  // namespace rio
