// rio_sst_keys.h — keys of a loaded table on the device (rio_sst_view): the clamped accessors, the 8-byte
// big-endian key prefix, bytes.Compare and the prefix-probed binary search. Shared by the merge plan
// (rio_compact.hip) and the point lookup (rio_bloom.hip). Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_device.h"
#include "rio_dev_util.h"

namespace rio {

constexpr uint64_t kEntryMask = (1ull << RIO_MERGE_ENTRY_BITS) - 1;

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

}  // namespace rio
