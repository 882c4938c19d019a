// rio_sst_keys.h — keys and values of a loaded table on the device (rio_sst_view): the clamped accessors, the
// 8-byte big-endian key prefix, bytes.Compare and the prefix-probed binary search, and a key's FNV-1 hash with
// the filter test on it. Shared by the merge plan (rio_compact.hip), the point lookup (rio_bloom.hip) and the
// stack of tables (rio_stack.hip); the stack's status rules also by the combined read (rio_db.hip). Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_device.h"
#include "rio_dev_util.h"

namespace rio {

constexpr uint64_t kEntryMask = (1ull << RIO_MERGE_ENTRY_BITS) - 1;

// value i of a view: [b, e) clamped to the data arena
__device__ __forceinline__ bool value_at(const rio_sst_view& v, uint64_t i, uint64_t& b, uint64_t& e) {
    const uint64_t o0 = v.data_off[i], o1 = v.data_off[i + 1];
    b = umin(o0, v.data_bytes);
    e = umin(umax(o1, b), v.data_bytes);
    return b == o0 && e == o1;
}

struct Key {
    const uint8_t* p;
    uint64_t len;
    uint64_t pfx;
};

// key i of a view, clamped to the index arena; ok = false when the clamp changed it
__device__ __forceinline__ Key key_at(const rio_sst_view& v, uint64_t i, bool& ok) {
    const uint64_t o = v.key_off[i], l = v.key_len[i];
    const uint64_t co = umin(o, v.index_bytes), cl = umin(l, v.index_bytes - co);
    ok = co == o && cl == l;
    return Key{v.index + co, cl, 0};
}
__device__ __forceinline__ uint64_t key_prefix(const Key& k) {
    uint64_t p = 0;
    for (uint32_t b = 0; b < 8; b++) p = (p << 8) | (b < k.len ? k.p[b] : 0u);
    return p;
}

// bytes.Compare(a, b) given both keys' prefixes: < 0, 0, > 0
__device__ __forceinline__ int key_cmp(const Key& a, const Key& b) {
    if (a.pfx != b.pfx) return a.pfx < b.pfx ? -1 : 1;
    // equal zero-padded prefixes: the first min(8, la, lb) bytes are equal
    const uint64_t m = umin(a.len, b.len);
    for (uint64_t k = umin(m, (uint64_t)8); k < m; k++) {
        const uint32_t x = a.p[k], y = b.p[k];
        if (x != y) return x < y ? -1 : 1;
    }
    return a.len == b.len ? 0 : (a.len < b.len ? -1 : 1);
}

// bytes.Compare(key `mid` of table v, k): the probe is the 8-byte prefix load; the key's offset, length
// and bytes are read only when the two prefixes are equal
__device__ __forceinline__ int entry_cmp(const rio_sst_view& v, const uint64_t* pfx, uint64_t mid, const Key& k) {
    const uint64_t p = pfx[mid];
    if (p != k.pfx) return p < k.pfx ? -1 : 1;
    bool ok;
    Key m = key_at(v, mid, ok);
    m.pfx = p;
    return key_cmp(m, k);
}

// lower (upper = false) or upper bound of key k among table u's keys; every probe stays in [0, n)
template <bool kUpper>
__device__ __forceinline__ uint64_t bound(const rio_sst_view& v, const uint64_t* pfx, const Key& k) {
    uint64_t lo = 0, hi = v.n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const int c = entry_cmp(v, pfx, mid, k);
        if (kUpper ? c <= 0 : c < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a source word read back from a buffer: table and entry clamped to what exists (false: no such entry)
__device__ __forceinline__ bool entry_of(const rio_sst_view* views, uint32_t T, uint64_t word, const rio_sst_view*& v,
                                         uint64_t& i) {
    const uint64_t t = word >> RIO_MERGE_ENTRY_BITS;
    v = &views[t < T ? t : 0];
    i = word & kEntryMask;
    if (t >= T || i >= v->n) {
        i = 0;
        return false;
    }
    return true;
}

// status byte (RIO_GET_*) and value length of a lookup's source word over a stack's tables: what Get returns for
// the entry (sstable_reader.go:67-114). stored = the tables' stored-checksum pointers; check_crc is
// EnableHashCheckOnReads. k_stack_value_len's rules (rio_stack.hip), which k_db_value_len (rio_db.hip) starts from
__device__ __forceinline__ void table_status(const rio_sst_view* views, const uint64_t* const* stored_of, uint32_t T,
                                             uint32_t check_crc, uint64_t word, uint32_t& status, uint64_t& len) {
    status = RIO_GET_NOT_FOUND;
    const rio_sst_view* v;
    uint64_t e;
    if (entry_of(views, T, word, v, e)) {
        const uint8_t fl = v->flags[e];
        const uint64_t* stored = stored_of[word >> RIO_MERGE_ENTRY_BITS];  // entry_of: the table exists
        if (fl & (RIO_FLAG_CORRUPT | RIO_FLAG_EOF)) {
            status = RIO_GET_HOST;
        } else if (check_crc && stored && stored[e] != 0 && stored[e] != v->crc[e]) {
            status = RIO_GET_HOST;
        } else if (fl & RIO_FLAG_NIL) {
            status = RIO_GET_NIL;
        } else {
            uint64_t vb, ve;
            value_at(*v, e, vb, ve);
            len = ve - vb;
            status = RIO_GET_VALUE;
        }
    }
}

constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;

typedef uint64_t __attribute__((aligned(1))) u64u;

// FNV-1 (64 bit) of p[0, len); `room` >= len bytes are readable from p. Whole 8-byte unaligned loads while 8
// bytes are readable (the last one may pass the key's end by up to 7 bytes, inside the arena: those bytes are
// not hashed), single bytes for a tail at the arena's very end
__device__ __forceinline__ uint64_t fnv1(const uint8_t* p, uint64_t len, uint64_t room) {
    uint64_t h = kFnvBasis, b = 0;
    for (; b < len && b + 8 <= room; b += 8) {
        uint64_t w = *reinterpret_cast<const u64u*>(p + b);
        const uint32_t cnt = (uint32_t)umin(len - b, (uint64_t)8);
        for (uint32_t j = 0; j < cnt; j++) {
            h = (h * kFnvPrime) ^ (w & 0xFF);
            w >>= 8;
        }
    }
    for (; b < len; b++) h = (h * kFnvPrime) ^ p[b];
    return h;
}

// all k probes of hash h set in filter f; hk holds the filter's min(k, RIO_BLOOM_MAX_K) hash keys (LDS or global)
__device__ __forceinline__ bool filter_contains(const rio_bloom_view& f, const uint64_t* hk, uint64_t h) {
    const uint32_t k = umin(f.k, RIO_BLOOM_MAX_K);
    for (uint32_t j = 0; j < k; j++) {
        const uint64_t idx = (h ^ hk[j]) % f.m;
        if (!((f.bits[idx >> 6] >> (idx & 63)) & 1)) return false;
    }
    return true;
}

}  // namespace rio
