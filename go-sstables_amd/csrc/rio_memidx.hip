// rio_memidx.hip — a memstore's op log made searchable in place, and MemStore.Get over up to two of them
// (memstore/memstore.go:107-123 through simpledb/rw_memstore.go:22-36: the write store, and only on its
// KeyNotFound the read store). The log stays where WriteBatch.upload, the WAL recovery or the memstore's flush
// left it; the index is 16 bytes per distinct key and points into it: no key and no value is copied.
//
// Build, after rio_sst_flush_plan's check, sort and keep stages under RIO_FLUSH_WITH_TOMBSTONES (rio_flush.hip: src
// = the ops ordered by (key, op index), keep = the last op of every key, nil ones included):
//   hipcub::DeviceSelect::Flagged  order = src compacted by keep: the latest op of every distinct key, keys ascending
//   k_mem_seal     one lane: a rejected log (RIO_MERGE_R_UNSORTED set) gets n_keys = RIO_MERGE_R_N_OUT = 0
//   k_mem_prefix   one lane per distinct key: pfx[j] = key_prefix of op order[j] (rio_sst_keys.h)
// Lookup:
//   k_mem_lookup   one lane per query in a grid-stride loop: the query's prefix once, then the stores from newest
//                  to oldest; per store a binary search over n_keys (read from the result block in device memory,
//                  clamped to ops.n) that probes pfx[mid] alone and reads order[mid], the op's key range and its
//                  bytes only when the prefixes are equal; the first store that holds the key answers, nil op or
//                  not. Like k_stack_lookup a chain of ceil(log2 n_keys) dependent 8-byte loads per store, hidden
//                  by the other waves of the CU, not by anything inside the lane; the equal-prefix step adds two
//                  more dependent loads (order, then key_off) before the key bytes, where a table has one
// Every index read back from a buffer is clamped (n_keys to ops.n, an op to [0, ops.n), ranges to their arenas):
// a wrong input gives ~0 or a wrong op, never an out-of-range access. Nothing past key_bytes of the query arena
// is read.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_ops_keys.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {

// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loops again
constexpr uint64_t kMemGridCap = 2048;

// order[j] of an index, clamped to the log
__device__ __forceinline__ uint64_t order_at(const rio_mem_index& I, uint64_t j) {
    const uint64_t op = I.order[j] & kEntryMask;
    return op < I.ops.n ? op : 0;
}

// the op of index I that holds q, or ~0
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

}  // namespace

__global__ void k_mem_seal(uint64_t* result) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && result[RIO_MERGE_R_UNSORTED] != ~0ull) result[RIO_MERGE_R_N_OUT] = 0;
}

__global__ void __launch_bounds__(256) k_mem_prefix(MemBuildParams P) {
    const uint64_t n = umin(P.result[RIO_MERGE_R_N_OUT], P.ops.n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint64_t w = P.order[j] & kEntryMask;
        P.pfx[j] = key_prefix(op_key(P.ops, w < P.ops.n ? w : 0));
    }
}

__global__ void __launch_bounds__(256) k_mem_lookup(MemLookupParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        const uint64_t a = P.key_off[i], b = P.key_off[i + 1];
        const uint64_t off = umin(a, P.key_bytes);
        const uint64_t e = umin(umax(b, off), P.key_bytes);
        Key q{P.keys + off, e - off, 0};
        q.pfx = key_prefix(q);
        uint64_t found = ~0ull;
        if (P.n_idx > 1) {
            const uint64_t op = find_in_mem(P.i1, q);
            if (op != ~0ull) found = (1ull << RIO_MERGE_ENTRY_BITS) | op;
        }
        if (found == ~0ull) found = find_in_mem(P.i0, q);  // store 0: the word is the op
        P.src[i] = found;
    }
}

namespace {
unsigned grid_for(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, kMemGridCap));
}
}  // namespace

size_t mem_index_cub_bytes(uint64_t n) {
    size_t b = 0;
    if (hipcub::DeviceSelect::Flagged(nullptr, b, (const uint64_t*)nullptr, (const uint8_t*)nullptr, (uint64_t*)nullptr,
                                      (uint64_t*)nullptr, (int)n) != hipSuccess)
        return 0;
    return b;
}

// after launch_flush_plan(P.ops -> P.src, P.keep, P.result) on the same stream; P.ops.n > 0
hipError_t launch_mem_index(const MemBuildParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    size_t tb = cub_bytes;
    const hipError_t e = hipcub::DeviceSelect::Flagged(cub_tmp, tb, P.src, P.keep, P.order, P.n_sel, (int)P.ops.n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mem_seal, dim3(1), dim3(64), 0, s, P.result);
    hipLaunchKernelGGL(k_mem_prefix, dim3(grid_for(P.ops.n)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_mem_lookup(const MemLookupParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_mem_lookup, dim3(grid_for(P.n)), dim3(256), 0, s, P);
    return hipGetLastError();
}

}  // namespace rio
