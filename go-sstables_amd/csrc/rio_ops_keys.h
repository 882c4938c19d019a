// rio_ops_keys.h — keys and values of an op log on the device (rio_ops_view): the clamped ranges of an op's key and
// value, an op's key as the Key the table searches compare (rio_sst_keys.h), and the binary search of a memstore
// index for a key. Shared by the flush plan (rio_flush.hip), the memstore index and its lookup (rio_memidx.hip), the
// size scan (rio_memsize.hip) and the combined read (rio_db.hip).
// Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_sst_keys.h"

namespace rio {

// key of op i: offset and length clamped to the arena and to max_len; false when the clamp changed them
__device__ __forceinline__ bool key_range(const rio_ops_view& o, uint64_t max_len, uint64_t i, uint64_t& off,
                                          uint64_t& len) {
    const uint64_t a = o.key_off[i], b = o.key_off[i + 1];
    off = umin(a, o.key_bytes);
    const uint64_t e = umin(umax(b, off), o.key_bytes);
    len = umin(e - off, max_len);
    return off == a && e == b && len == e - off;
}
// value of op i: [b, e) clamped to the value arena
__device__ __forceinline__ bool value_range(const rio_ops_view& o, uint64_t i, uint64_t& b, uint64_t& e) {
    const uint64_t o0 = o.val_off[i], o1 = o.val_off[i + 1];
    b = umin(o0, o.value_bytes);
    e = umin(umax(o1, b), o.value_bytes);
    return b == o0 && e == o1;
}

// key of op i (i < o.n) clamped to the arena, without its prefix
__device__ __forceinline__ Key op_key(const rio_ops_view& o, uint64_t i) {
    uint64_t off, len;
    key_range(o, ~0ull, i, off, len);
    return Key{o.keys + off, len, 0};
}

// the distinct keys of an index: the build's count read from device memory, clamped to the log's length
__device__ __forceinline__ uint64_t mem_n_keys(const rio_mem_index& I) {
    return I.ops.n ? umin(I.result[RIO_MERGE_R_N_OUT], I.ops.n) : 0;
}

// order[j] of an index, clamped to the log
__device__ __forceinline__ uint64_t order_at(const rio_mem_index& I, uint64_t j) {
    const uint64_t op = I.order[j] & kEntryMask;
    return op < I.ops.n ? op : 0;
}

// the op of index I that holds q, or ~0 (the probe of k_mem_lookup and of k_size_delta)
__device__ __forceinline__ uint64_t find_in_mem(const rio_mem_index& I, const Key& q) {
    uint64_t lo = 0, hi = mem_n_keys(I);
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t p = I.pfx[mid];
        int c;
        if (p != q.pfx) {
            c = p < q.pfx ? -1 : 1;
        } else {
            const uint64_t op = order_at(I, mid);
            Key m = op_key(I.ops, op);
            m.pfx = p;
            c = key_cmp(m, q);
            if (c == 0) return op;
        }
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return ~0ull;
}

// a memstore source word read back from a buffer: store and op clamped to what exists (false: no such op).
// The stores are named one by one: a by-value array indexed at run time would go through scratch memory
__device__ __forceinline__ bool mem_op_of(const rio_mem_index& i0, const rio_mem_index& i1, uint32_t n_idx, uint64_t word,
                                          const rio_mem_index*& I, uint64_t& op) {
    const uint64_t s = word >> RIO_MERGE_ENTRY_BITS;
    I = (s == 1 && n_idx > 1) ? &i1 : &i0;
    op = word & kEntryMask;
    if (s >= n_idx || op >= I->ops.n) {
        op = 0;
        return false;
    }
    return true;
}

}  // namespace rio
