// rio_memsize.hip — the memstore's size estimate after every op of a batch, and the op at which db.PutBytes would
// rotate (simpledb/db.go:299: memStore.EstimatedSizeInBytes() > memstoreMaxSize, checked after every put and after
// no delete, db.go:311-347). The estimate is running state (memstore/memstore.go:119-178 through
// simpledb/rw_memstore.go:48-63): what an op adds depends on whether the write store holds its key at that moment
// and with which value. The latest earlier op of the same key is the op's predecessor in the flush plan's order
// (rio_flush.hip: the ops by (key, op index)) while that order stays inside the batch, and the write store's entry
// for the first op of every key; so the deltas need no sequential pass and the sizes are their sum in op order.
//
// After rio_sst_flush_plan's check, sort and keep stages over the batch under RIO_FLUSH_WITH_TOMBSTONES (src = the
// ops ordered by (key, op index), keep = the last op of every key):
//   k_size_delta   one lane per sorted position p in a grid-stride loop: the predecessor of op src[p] is src[p - 1]
//                  when that is not the last op of its key, else the store's op for the key (find_in_mem,
//                  rio_ops_keys.h: the lookup's probe) or none. delta[op], mod 2^64:
//                    put,    key unknown   len(key) + len(value)       memstore.go:137-138
//                    put,    key known     len(value) - len(previous)  memstore.go:133-135 (a tombstone's length is 0)
//                    delete, key unknown   len(key)                    rw_memstore.go:50-51 -> memstore.go:172-175
//                    delete, key known     - len(previous)             memstore.go:158
//                  size0 rides on op 0's delta. A chain of ceil(log2 n_keys) dependent loads per first op of a key,
//                  as in k_mem_lookup; later ops of a key read two neighbours
//   hipcub::DeviceScan::InclusiveSum   size[i] = the raw estimatedSize after op i
//   k_size_cut     one lane per op in a grid-stride loop: the first put whose scaled size passes max_size; the
//                  minimum per lane, then per block (LDS), then one global atomicMin per block
//   k_size_seal    one lane: the result block (n = 0 runs this kernel alone)
// The scaled size is Go's uint64(1.15 * float32(size)) (memstore.go:182): the u64 -> f32 conversion rounds to
// nearest even, the product is one float32 multiply by float32(1.15), the conversion back truncates. A product of
// 2^64 and more saturates here (Go leaves that conversion to the platform).
// Every index read back from a buffer is clamped (an op to the batch or to the store's log, n_keys to the store's
// ops.n, ranges to their arenas, the cut to the batch): a wrong input gives wrong words, never an out-of-range access.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_ops_keys.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {

// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loops again
constexpr uint64_t kSizeGridCap = 2048;

__device__ __forceinline__ uint64_t batch_op(const MemSizeParams& P, uint64_t p) {
    const uint64_t op = P.src[p];
    return op < P.batch.n ? op : 0;
}
// the value length an op leaves behind: 0 for a nil op
__device__ __forceinline__ uint64_t left_len(const rio_ops_view& o, uint64_t op) {
    uint64_t vb, ve;
    value_range(o, op, vb, ve);
    return (o.flags[op] & RIO_FLAG_NIL) ? 0 : ve - vb;
}
// uint64(1.15 * float32(size)) > max_size
__device__ __forceinline__ bool over_limit(uint64_t size, uint64_t max_size) {
    const float f = 1.15f * __ull2float_rn(size);
    const uint64_t est = f >= 18446744073709551616.0f ? ~0ull : (uint64_t)f;
    return est > max_size;
}

}  // namespace

__global__ void __launch_bounds__(256) k_size_delta(MemSizeParams P) {
    const uint64_t n = P.batch.n, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (p == 0) *P.cut = ~0ull;
        const uint64_t op = batch_op(P, p);
        uint64_t off, klen;
        key_range(P.batch, ~0ull, op, off, klen);
        bool known = false;
        uint64_t prev = 0;
        if (p > 0 && !P.keep[p - 1]) {  // position p - 1 holds the same key: its op came just before this one
            known = true;
            prev = left_len(P.batch, batch_op(P, p - 1));
        } else if (P.store.ops.n) {
            Key q{P.batch.keys + off, klen, 0};
            q.pfx = key_prefix(q);
            const uint64_t s_op = find_in_mem(P.store, q);
            if (s_op != ~0ull) {
                known = true;
                prev = left_len(P.store.ops, s_op);
            }
        }
        const uint64_t mine = left_len(P.batch, op);
        uint64_t d;
        if (P.batch.flags[op] & RIO_FLAG_NIL)
            d = known ? 0 - prev : klen;
        else
            d = known ? mine - prev : klen + mine;
        P.delta[op] = d + (op == 0 ? P.size0 : 0);
    }
}

__global__ void __launch_bounds__(256) k_size_cut(MemSizeParams P) {
    const uint64_t n = P.batch.n, stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t first = ~0ull;  // this lane's first over-limit put: its ops ascend
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n && first == ~0ull; i += stride)
        if (!(P.batch.flags[i] & RIO_FLAG_NIL) && over_limit(P.size[i], P.max_size)) first = i;
    __shared__ unsigned long long s_min;
    if (threadIdx.x == 0) s_min = ~0ull;
    __syncthreads();
    if (first != ~0ull) atomicMin(&s_min, (unsigned long long)first);
    __syncthreads();
    if (threadIdx.x == 0 && s_min != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(P.cut), s_min);
}

__global__ void k_size_seal(MemSizeParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t n = P.batch.n;
    uint64_t* R = P.result;
    uint64_t bad = n ? P.plan[RIO_MERGE_R_UNSORTED] : ~0ull;
    if (bad != ~0ull) bad = umin(bad, n - 1);
    if (P.store.ops.n && P.store.result[RIO_MERGE_R_UNSORTED] != ~0ull) bad = 0;
    uint64_t cut = ~0ull, size = P.size0, key_end = 0, value_end = 0;
    if (n) {
        cut = *P.cut;
        if (cut >= n) cut = ~0ull;
        const uint64_t last = cut != ~0ull ? cut : n - 1;
        size = P.size[last];
        key_end = umin(P.batch.key_off[last + 1], P.batch.key_bytes);
        value_end = umin(P.batch.val_off[last + 1], P.batch.value_bytes);
    }
    for (uint32_t k = 0; k < RIO_SIZE_RESULT_WORDS; k++) R[k] = 0;
    R[RIO_SIZE_R_CUT] = cut;
    R[RIO_SIZE_R_SIZE] = size;
    R[RIO_SIZE_R_KEY_END] = key_end;
    R[RIO_SIZE_R_VALUE_END] = value_end;
    R[RIO_SIZE_R_FIRST_BAD] = bad;
}

size_t mem_size_cub_bytes(uint64_t n) {
    size_t b = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n) != hipSuccess)
        return 0;
    return b;
}

// after launch_flush_plan(P.batch -> P.src, P.keep, P.plan) on the same stream; P.batch.n = 0 needs no plan
hipError_t launch_mem_size(const MemSizeParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    const uint64_t n = P.batch.n;
    if (n) {
        hipLaunchKernelGGL(k_size_delta, dim3(grid_for(n, 256, kSizeGridCap)), dim3(256), 0, s, P);
        size_t tb = cub_bytes;
        const hipError_t e = hipcub::DeviceScan::InclusiveSum(cub_tmp, tb, (const uint64_t*)P.delta, P.size, (int)n, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_size_cut, dim3(grid_for(n, 256, kSizeGridCap)), dim3(256), 0, s, P);
    }
    hipLaunchKernelGGL(k_size_seal, dim3(1), dim3(64), 0, s, P);
    return hipGetLastError();
}

}  // namespace rio
