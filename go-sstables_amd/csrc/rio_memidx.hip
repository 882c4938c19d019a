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
//
// Extend (rio_mem_index_extend): the index A of ops [0, n_old) and the ops [n_old, n) behind them give the index
// of the whole log without sorting the old ops again. The tail goes through the build's own stages as a sub-view
// (offsets are absolute: key_off + n_old over the same arenas) into B, an index with op words relative to n_old;
// then
//   k_mem_rank     one lane per B entry: binary search over A by prefix, the full keys on equal prefixes (find_in_mem's
//                  probe); lb[j] = A keys below B[j], eq[j] = A[lb[j]] is B[j]'s key. Lanes from nB to t write
//                  lb = nA, eq = 0: the scan and the upper-bound searches run over t + 1 items, a host constant
//   hipcub::DeviceScan::ExclusiveSum   e = scan of eq: e[j] = A keys the tail rewrote before B[j], e[nB] all of them
//   k_mem_place    one lane per A and per B entry: B[j] to lb[j] + j - e[j]; A[i], with u = the B entries whose lb is
//                  <= i (an upper-bound search over lb, nB words), dropped when B[u - 1] is its key, else to
//                  i + u - e[u]. Order word and prefix move together into the merged copy (context scratch); a
//                  dropped entry's key length, value length and nil flag are summed per lane, then per block (LDS),
//                  then one global atomic per block and sum
//   k_mem_copy_back  the merged copy into order / pfx, each op word clamped to the log
//   k_mem_extend_seal  one lane: the result words (A's sums less the dropped entries' plus B's; n_keys = nA + nB -
//                  e[nB]; the first rejected op of the two), then k_mem_seal's rule
// nA is clamped to n_old, nB to t, an A op to [0, n_old), a B op to [n_old, n), a position to [0, n).
//
// k_ops_rebase (rio_ops_append): one lane per op of a batch, its end offsets moved behind a log's.
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
constexpr uint64_t kMemGridCap = 2048;

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
    hipLaunchKernelGGL(k_mem_prefix, dim3(grid_for(P.ops.n, 256, kMemGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_mem_lookup(const MemLookupParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_mem_lookup, dim3(grid_for(P.n, 256, kMemGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

// ---- extend ----------------------------------------------------------------------------------------------------

namespace {

__device__ __forceinline__ uint64_t ext_n_a(const MemExtendParams& P) { return umin(P.result[RIO_MERGE_R_N_OUT], P.n_old); }
__device__ __forceinline__ uint64_t ext_n_b(const MemExtendParams& P) { return umin(P.b_result[RIO_MERGE_R_N_OUT], P.t); }
// the op of A's entry i, clamped to the old ops; of B's entry j, clamped to the tail
__device__ __forceinline__ uint64_t ext_a_op(const MemExtendParams& P, uint64_t i) {
    const uint64_t op = P.order[i] & kEntryMask;
    return op < P.n_old ? op : 0;
}
__device__ __forceinline__ uint64_t ext_b_op(const MemExtendParams& P, uint64_t j) {
    const uint64_t op = P.b_order[j] & kEntryMask;
    return P.n_old + (op < P.t ? op : 0);
}

}  // namespace

__global__ void __launch_bounds__(256) k_mem_rank(MemExtendParams P) {
    const uint64_t nA = ext_n_a(P), nB = ext_n_b(P);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= P.t; j += stride) {
        if (j == 0)
            for (uint32_t k = 0; k < 4; k++) P.drop[k] = 0;
        uint64_t lo = nA, hit = 0;
        if (j < nB) {
            Key q = op_key(P.ops, ext_b_op(P, j));
            q.pfx = P.b_pfx[j];
            lo = 0;
            uint64_t hi = nA;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                const uint64_t p = P.pfx[mid];
                int c;
                if (p != q.pfx) {
                    c = p < q.pfx ? -1 : 1;
                } else {
                    Key m = op_key(P.ops, ext_a_op(P, mid));
                    m.pfx = p;
                    c = key_cmp(m, q);
                    if (c == 0) {
                        lo = mid;
                        hit = 1;
                        break;
                    }
                }
                if (c < 0) lo = mid + 1; else hi = mid;
            }
        }
        P.lb[j] = lo;
        P.eq[j] = hit;
    }
}

__global__ void __launch_bounds__(256) k_mem_place(MemExtendParams P) {
    const uint64_t nA = ext_n_a(P), nB = ext_n_b(P), n = P.ops.n;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t d_cnt = 0, d_val = 0, d_nil = 0, d_key = 0;  // this lane's dropped A entries
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < nA + nB; x += stride) {
        uint64_t pos, word, pfx;
        if (x < nA) {
            uint64_t u = 0, hi = nB;  // B entries whose lower bound is at or before x
            while (u < hi) {
                const uint64_t mid = u + ((hi - u) >> 1);
                if (P.lb[mid] <= x) u = mid + 1; else hi = mid;
            }
            word = ext_a_op(P, x);
            if (u > 0 && P.eq[u - 1] && P.lb[u - 1] == x) {  // the tail rewrote this key: B[u - 1] stands for it
                uint64_t off, len, vb, ve;
                key_range(P.ops, ~0ull, word, off, len);
                value_range(P.ops, word, vb, ve);
                d_cnt++;
                d_key += len;
                if (P.ops.flags[word] & RIO_FLAG_NIL) d_nil++; else d_val += ve - vb;
                continue;
            }
            pos = x + u - umin(P.e[u], u);
            pfx = P.pfx[x];
        } else {
            const uint64_t j = x - nA;
            pos = umin(P.lb[j], nA) + j - umin(P.e[j], j);
            word = ext_b_op(P, j);
            pfx = P.b_pfx[j];
        }
        pos = umin(pos, n - 1);
        P.m_order[pos] = word;
        P.m_pfx[pos] = pfx;
    }
    __shared__ unsigned long long s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __syncthreads();
    if (d_cnt) {
        atomicAdd(&s_sum[0], (unsigned long long)d_cnt);
        if (d_val) atomicAdd(&s_sum[1], (unsigned long long)d_val);
        if (d_nil) atomicAdd(&s_sum[2], (unsigned long long)d_nil);
        if (d_key) atomicAdd(&s_sum[3], (unsigned long long)d_key);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_sum[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(&P.drop[threadIdx.x]), s_sum[threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_mem_copy_back(MemExtendParams P) {
    const uint64_t nA = ext_n_a(P), nB = ext_n_b(P), n = P.ops.n;
    const uint64_t nk = umin(nA + nB - umin(P.e[nB], nB), n);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nk; p += stride) {
        const uint64_t w = P.m_order[p];
        P.order[p] = w < n ? w : 0;
        P.pfx[p] = P.m_pfx[p];
    }
}

__global__ void k_mem_extend_seal(MemExtendParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t nA = ext_n_a(P), nB = ext_n_b(P);
    uint64_t* R = P.result;
    const uint64_t* B = P.b_result;
    // the first rejected op of the whole log: the old ops come first
    uint64_t bad = R[RIO_MERGE_R_UNSORTED];
    if (bad == ~0ull && B[RIO_MERGE_R_UNSORTED] != ~0ull) bad = P.n_old + umin(B[RIO_MERGE_R_UNSORTED], P.t - 1);
    R[RIO_MERGE_R_N_OUT] = bad != ~0ull ? 0 : umin(nA + nB - umin(P.e[nB], nB), P.ops.n);
    R[RIO_MERGE_R_VALUE_BYTES] = R[RIO_MERGE_R_VALUE_BYTES] - P.drop[1] + B[RIO_MERGE_R_VALUE_BYTES];
    R[RIO_MERGE_R_NULL_VALUES] = R[RIO_MERGE_R_NULL_VALUES] - P.drop[2] + B[RIO_MERGE_R_NULL_VALUES];
    R[RIO_MERGE_R_KEY_BYTES] = R[RIO_MERGE_R_KEY_BYTES] - P.drop[3] + B[RIO_MERGE_R_KEY_BYTES];
    R[RIO_MERGE_R_FIRST_DUP] = ~0ull;
    R[RIO_MERGE_R_UNSORTED] = bad;
}

__global__ void __launch_bounds__(256) k_ops_rebase(OpsRebaseParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        if (i == 0 && P.log_n == 0) P.key_off[0] = P.val_off[0] = 0;
        P.key_off[P.log_n + 1 + i] = P.log_key_bytes + umin(P.b_key_off[i + 1], P.b_key_bytes);
        P.val_off[P.log_n + 1 + i] = P.log_value_bytes + umin(P.b_val_off[i + 1], P.b_value_bytes);
    }
}

size_t mem_extend_cub_bytes(uint64_t t) {
    return std::max(scan_cub_bytes(t), mem_index_cub_bytes(t));
}

// after the tail's launch_flush_plan and launch_mem_index (into P.b_order, P.b_pfx, P.b_result) on the same stream
hipError_t launch_mem_extend(const MemExtendParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_mem_rank, dim3(grid_for(P.t + 1, 256, kMemGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.eq, P.e, P.t, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mem_place, dim3(grid_for(P.ops.n, 256, kMemGridCap)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_mem_copy_back, dim3(grid_for(P.ops.n, 256, kMemGridCap)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_mem_extend_seal, dim3(1), dim3(64), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_ops_rebase(const OpsRebaseParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_ops_rebase, dim3(grid_for(P.n, 256, kMemGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

}  // namespace rio
