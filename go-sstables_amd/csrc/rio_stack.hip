// rio_stack.hip — a stack of loaded tables on the device: SuperSSTableReader.Contains / Get
// (sstables/super_sstable_reader.go:18-49: the readers from newest to oldest, the first table that holds the
// key answers) for a batch of query keys, the values of the entries found, the cut points of
// ScanStartingAt / ScanRange for every table (slice_key_index.go:49-70), and the keys of a plan's survivors
// (what a scan returns beside the values of rio_sst_merge_gather). The stack's tables (views, prefix
// pointers, filters, stored-checksum pointers) are device arrays of T entries that the stack owns; table t is
// read at a wave-uniform address.
//
//   k_stack_lookup      one lane per query: FNV-1 of the query once (it does not depend on the table), then
//                       t = T-1 .. 0: the optional filter gate with table t's hash keys, bound<false> over its
//                       prefixes, the equality test; the lane stops at its first hit. The lookup is a chain of
//                       dependent probes: ungated ceil(log2 n_t) 8-byte prefix loads per table down to the one
//                       that holds the key, gated up to k_t filter loads instead for each table that rejects it.
//                       The hash keys are read from global memory (512 bytes per table, the same for every
//                       lane: cached), so a lane that has found its key leaves the table loop on its own. The
//                       other shape (hash keys staged in LDS per table, the table loop block-uniform with a
//                       found predicate and a block-wide skip) was measured beside it and not kept: DESIGN.md
//                       §4; its text is in profiles/r10/README.md
//   k_stack_value_len   one lane per query: status byte (RIO_GET_*) and value length, the scan's input
//   k_stack_value_copy<G>  G lanes per value (16 under kLongItem bytes, a wave for the others): copy_ranges
//                       (rio_seg_copy.h)
//   k_stack_bounds      one lane per (key, table): lower or upper bound
//   k_keys_len / k_keys_copy<G>  key lengths of a plan's survivors, then (after a scan) their bytes: copy_ranges
// Every table and entry number read from a buffer is clamped (entry_of), every key and value range is clamped
// to its arena, every store is checked against its capacity: a wrong input gives ~0, RIO_GET_NOT_FOUND or wrong
// bytes, never an out-of-range access.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {

// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loops again
constexpr uint64_t kStackGridCap = 2048;

// query i of the arena: clamped to [0, key_bytes); room = bytes readable from its first byte
__device__ __forceinline__ Key query_key(const StackParams& P, uint64_t i, uint64_t& room) {
    const uint64_t a = P.key_off[i], b = P.key_off[i + 1];
    const uint64_t off = umin(a, P.key_bytes);
    const uint64_t e = umin(umax(b, off), P.key_bytes);
    room = P.key_bytes - off;
    Key q{P.keys + off, e - off, 0};
    q.pfx = key_prefix(q);
    return q;
}

// the entry of table t that holds q, as a source word, or ~0
__device__ __forceinline__ uint64_t find_in(const StackParams& P, uint32_t t, const Key& q) {
    const rio_sst_view& v = P.views[t];
    const uint64_t* pfx = P.pfx[t];
    const uint64_t lb = bound<false>(v, pfx, q);
    if (lb < v.n && entry_cmp(v, pfx, lb, q) == 0) return ((uint64_t)t << RIO_MERGE_ENTRY_BITS) | lb;
    return ~0ull;
}

}  // namespace

__global__ void __launch_bounds__(256) k_stack_lookup(StackParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        uint64_t room;
        const Key q = query_key(P, i, room);
        const uint64_t h = P.flag ? fnv1(q.p, q.len, room) : 0;
        uint64_t found = ~0ull;
        for (uint32_t t = P.T; t-- > 0;) {
            const rio_bloom_view& f = P.filters[t];
            if (P.flag && f.bits && !filter_contains(f, f.hash_keys, h)) continue;
            found = find_in(P, t, q);
            if (found != ~0ull) break;
        }
        P.src[i] = found;
    }
}

// status and value length per query; position n holds the scan's last input, 0
__global__ void __launch_bounds__(256) k_stack_value_len(StackParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= P.n; i += stride) {
        uint64_t len = 0;
        if (i < P.n) {
            uint32_t status;
            table_status(P.views, P.stored, P.T, P.flag, P.src[i], status, len);
            P.status[i] = (uint8_t)status;
        }
        P.tmp[i] = len;
    }
}

// G lanes per value. kLong = false: values shorter than kLongItem; true: the others.
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_stack_value_copy(StackParams P) {
    copy_ranges<G, kLong>(P.n, P.val_off, P.values_cap, P.values, [&](uint64_t j, uint64_t len) __attribute__((always_inline)) -> const uint8_t* {
        const rio_sst_view* v;
        uint64_t i, vb, ve;
        if (!entry_of(P.views, P.T, P.src[j], v, i)) return nullptr;
        value_at(*v, i, vb, ve);
        return ve - vb == len ? v->data + vb : nullptr;
    });
}

__global__ void __launch_bounds__(256) k_stack_bounds(StackParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t total = P.n * P.T;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint64_t k = g / P.T;
        const uint32_t t = (uint32_t)(g % P.T);
        uint64_t room;
        const Key q = query_key(P, k, room);
        const rio_sst_view& v = P.views[t];
        P.pos[g] = P.flag ? bound<true>(v, P.pfx[t], q) : bound<false>(v, P.pfx[t], q);
    }
}

__global__ void __launch_bounds__(256) k_keys_len(KeysParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= P.n_out; j += stride) {
        uint64_t len = 0;
        const rio_sst_view* v;
        uint64_t i;
        if (j < P.n_out && entry_of(P.views, P.T, P.out_src[j], v, i)) {
            bool ok;
            len = key_at(*v, i, ok).len;
        }
        P.tmp[j] = len;
    }
}

template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_keys_copy(KeysParams P) {
    copy_ranges<G, kLong>(P.n_out, P.key_off, P.keys_cap, P.keys, [&](uint64_t j, uint64_t len) __attribute__((always_inline)) -> const uint8_t* {
        const rio_sst_view* v;
        uint64_t i;
        if (!entry_of(P.views, P.T, P.out_src[j], v, i)) return nullptr;
        bool ok;
        const Key k = key_at(*v, i, ok);
        return k.len == len ? k.p : nullptr;
    });
}

hipError_t launch_stack_lookup(const StackParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_stack_lookup, dim3(grid_for(P.n, 256, kStackGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_stack_value_plan(const StackParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_stack_value_len, dim3(grid_for(P.n + 1, 256, kStackGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.val_off, P.n, s);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_stack_value_copy(const StackParams& P, hipStream_t s) {
    launch_short_long(k_stack_value_copy<16, false>, k_stack_value_copy<64, true>, P.n, P, s);
    return hipGetLastError();
}

hipError_t launch_stack_bounds(const StackParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_stack_bounds, dim3(grid_for(P.n * P.T, 256, kStackGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_keys_gather(const KeysParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_keys_len, dim3(grid_for(P.n_out + 1, 256, kStackGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.key_off, P.n_out, s);
    if (e != hipSuccess) return e;
    if (P.n_out) launch_short_long(k_keys_copy<16, false>, k_keys_copy<64, true>, P.n_out, P, s);
    return hipGetLastError();
}

}  // namespace rio
