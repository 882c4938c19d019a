// rio_compact.hip — merge-compaction of loaded SSTables on the device: SSTableMerger.Merge /
// MergeCompact (sstables/sstable_merger.go:36-169) with ScanReduceLatestWins /
// ScanReduceLatestWinsSkipTombstones (super_sstable_reader.go:107-131), the value side of the
// output table (the arena rio_device_encode takes) and its IndexEntry records
// (sstable_writer.go:126-132). Input: T tables as the load leaves them in HBM (rio_sst_view).
//
// Plan: rank by search. The reference pops a heap of T iterators once per entry; here every entry
// computes its own merged position. Entry i of table t has key k; within the order (key, table
// position) exactly i entries of its own table, upper_bound_u(k) entries of every earlier table u and
// lower_bound_u(k) entries of every later table u come before it, so
//     pos = i + sum_{u<t} upper_bound_u(k) + sum_{u>t} lower_bound_u(k)
// is a bijection onto [0, N) when every table is strictly ascending. (T - 1) * ceil(log2 n) probes
// per entry, each one 8-byte load of a big-endian key prefix (k_merge_keys) and a byte compare only
// when two prefixes are equal. Lanes of a wave hold neighbouring keys of one table, so the first
// probes of their searches coincide (one cache line per wave) and the last ones fall into a few lines.
// The same searches decide survival: an entry wins its key group when no later table holds its key,
// and under RIO_MERGE_ALL its key repeats its predecessor's when an earlier table holds it.
// A merge-path partition would read every key once instead of log n times, but it needs the diagonal
// search per T-way split and a serial merge inside each partition over variable-length keys; rank by
// search is exact, has no serial part and no inter-block state.
//
//   k_merge_keys     one lane per input entry: key prefix; each table's strict order and the bounds of
//                    its key / value ranges are checked here, not trusted (RIO_MERGE_R_UNSORTED)
//   k_merge_rank     one lane per input entry: position, keep flag, the result block's sums
//   k_gather_select  survivors compacted by an exclusive scan of the keep flags: source word,
//                    value length, nil flag
//   k_gather_copy<G> G lanes per value (16 for values under kLongItem bytes, a wave for the others):
//                    copy_ranges (rio_seg_copy.h); nothing is read or written outside the value
//   k_entry_len / k_entry_write   IndexEntry sizes, then (after a scan) their bytes
// Every table and entry index read from a buffer is clamped before use (view_of / entry_of), every
// key and value range is clamped to its arena, and every store is checked against its capacity: a
// wrong input gives a status or wrong bytes, never an out-of-range access.
#include <hip/hip_runtime.h>
#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {

// the lane-per-entry kernels' grid: longer inputs go round the grid-stride loops again
constexpr uint64_t kMergeGridCap = 4096;

// table of input entry number g: the last t with base[t] <= g (base in LDS, base[T] = N > g)
__device__ __forceinline__ uint32_t table_of(const uint64_t* base, uint32_t T, uint64_t g) {
    uint32_t lo = 0, hi = T;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void load_base(uint64_t* s_base, const uint64_t* base, uint32_t T) {
    for (uint32_t k = threadIdx.x; k <= T; k += blockDim.x) s_base[k] = base[k];
    __syncthreads();
}

}  // namespace

__global__ void k_merge_init(uint64_t* r) {
    if (threadIdx.x < RIO_MERGE_RESULT_WORDS)
        r[threadIdx.x] = (threadIdx.x == RIO_MERGE_R_FIRST_DUP || threadIdx.x == RIO_MERGE_R_UNSORTED) ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(256) k_merge_keys(MergeParams P) {
    __shared__ uint64_t s_base[RIO_MERGE_MAX_TABLES + 1];
    load_base(s_base, P.base, P.T);
    unsigned long long* unsorted = reinterpret_cast<unsigned long long*>(&P.result[RIO_MERGE_R_UNSORTED]);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < P.N; g += stride) {
        const uint32_t t = table_of(s_base, P.T, g);
        const rio_sst_view& v = P.views[t];
        const uint64_t i = g - s_base[t];
        bool ok, okv;
        Key k = key_at(v, i, ok);
        k.pfx = key_prefix(k);
        P.pfx[g] = k.pfx;
        uint64_t vb, ve;
        okv = value_at(v, i, vb, ve);
        if (i) {
            bool okp;
            Key prev = key_at(v, i - 1, okp);
            prev.pfx = key_prefix(prev);
            ok = ok && key_cmp(prev, k) < 0;
        }
        if (!(ok && okv)) atomicMin(unsorted, (unsigned long long)t);
    }
}

__global__ void __launch_bounds__(256) k_merge_rank(MergeParams P) {
    __shared__ uint64_t s_base[RIO_MERGE_MAX_TABLES + 1];
    load_base(s_base, P.base, P.T);
    unsigned long long* R = reinterpret_cast<unsigned long long*>(P.result);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // the result block's sums: LDS atomics per round, then one global atomic per block, round and sum
    // (whole blocks iterate together for the barriers)
    __shared__ unsigned long long s_sum[4];
    const uint64_t rounds = (P.N + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t g = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
        __syncthreads();
        if (g < P.N) {
            const uint32_t t = table_of(s_base, P.T, g);
            const rio_sst_view& v = P.views[t];
            const uint64_t i = g - s_base[t];
            bool ok;
            Key k = key_at(v, i, ok);
            k.pfx = P.pfx[g];
            uint64_t pos = i;
            bool earlier = false, later = false;  // the key is also in a table before / after t
            for (uint32_t u = 0; u < P.T; u++) {
                if (u == t) continue;
                const rio_sst_view& w = P.views[u];
                const uint64_t* wp = P.pfx + s_base[u];
                if (u < t) {
                    const uint64_t ub = bound<true>(w, wp, k);
                    pos += ub;
                    if (ub) earlier = earlier || entry_cmp(w, wp, ub - 1, k) == 0;
                } else {
                    const uint64_t lb = bound<false>(w, wp, k);
                    pos += lb;
                    if (lb < w.n) later = later || entry_cmp(w, wp, lb, k) == 0;
                }
            }
            uint64_t vb, ve;
            value_at(v, i, vb, ve);
            const bool nil = (v.flags[i] & RIO_FLAG_NIL) != 0;
            const uint64_t vlen = nil ? 0 : ve - vb;
            bool keep;
            if (P.mode == RIO_MERGE_ALL) {
                keep = true;
                if (earlier) atomicMin(&R[RIO_MERGE_R_FIRST_DUP], (unsigned long long)pos);
            } else {
                // the entry of the highest table position is the group's value; a nil one drops the
                // group (sstable_merger.go:86,102), SkipTombstones also an empty one
                keep = !later && !nil && !(P.mode == RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES && vlen == 0);
            }
            // pos < N for any input: i < n_t and every bound is at most its table's n
            P.src[pos] = ((uint64_t)t << RIO_MERGE_ENTRY_BITS) | i;
            P.keep[pos] = keep ? 1 : 0;
            if (keep) {
                atomicAdd(&s_sum[0], 1ull);
                if (vlen) atomicAdd(&s_sum[1], (unsigned long long)vlen);
                if (nil) atomicAdd(&s_sum[2], 1ull);
                if (k.len) atomicAdd(&s_sum[3], (unsigned long long)k.len);
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

__global__ void __launch_bounds__(256) k_gather_flags(GatherParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= P.N; p += stride)
        P.tmp[p] = p < P.N && P.keep[p] ? 1 : 0;
}

// survivors in merged order: source word, nil flag, value length (into tmp, the next scan's input)
__global__ void __launch_bounds__(256) k_gather_select(GatherParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P.N; p += stride) {
        if (!P.keep[p]) continue;
        const uint64_t j = P.opos[p];
        if (j >= P.n_out) continue;  // a caller's n_out smaller than the plan's
        const uint64_t word = P.src[p];
        const rio_sst_view* v;
        uint64_t i, vb = 0, ve = 0;
        bool nil = true;
        if (entry_of(P.views, P.T, word, v, i)) {
            value_at(*v, i, vb, ve);
            nil = (v->flags[i] & RIO_FLAG_NIL) != 0;
        }
        P.out_src[j] = word;
        P.val_flags[j] = nil ? RIO_FLAG_NIL : 0;
        P.tmp[j] = nil ? 0 : ve - vb;
    }
}
// positions past the plan's count (a caller's n_out larger than it) hold empty values
__global__ void __launch_bounds__(256) k_gather_pad(GatherParams P) {
    const uint64_t have = P.opos[P.N];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = have + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= P.n_out; j += stride) {
        P.tmp[j] = 0;
        if (j < P.n_out) {
            P.out_src[j] = ~0ull;
            P.val_flags[j] = RIO_FLAG_NIL;
        }
    }
}

// G lanes per value. kLong = false: values shorter than kLongItem; true: the others.
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_gather_copy(GatherParams P) {
    copy_ranges<G, kLong>(P.n_out, P.val_off, P.values_cap, P.values, [&](uint64_t j, uint64_t len) __attribute__((always_inline)) -> const uint8_t* {
        const rio_sst_view* v;
        uint64_t i, vb, ve;
        if (!entry_of(P.views, P.T, P.out_src[j], v, i)) return nullptr;
        value_at(*v, i, vb, ve);
        return ve - vb == len ? v->data + vb : nullptr;
    });
}

__global__ void __launch_bounds__(256) k_entry_len(EntryParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= P.n_out; j += stride) {
        uint64_t len = 0;
        const rio_sst_view* v;
        uint64_t i;
        if (j < P.n_out && entry_of(P.views, P.T, P.out_src[j], v, i)) {
            bool ok;
            const Key k = key_at(*v, i, ok);
            len = pb_index_entry_len(k.len, P.file_off[j], v->crc[i]);
        }
        P.tmp[j] = len;
    }
}

__global__ void __launch_bounds__(256) k_entry_write(EntryParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < P.n_out; j += stride) {
        const uint64_t e0 = P.ent_off[j], e1 = P.ent_off[j + 1];
        if (e1 > P.entries_cap || e1 < e0) continue;
        const rio_sst_view* v;
        uint64_t i;
        if (!entry_of(P.views, P.T, P.out_src[j], v, i)) continue;
        bool ok;
        const Key k = key_at(*v, i, ok);
        const uint64_t vo = P.file_off[j], cs = v->crc[i];
        if (pb_index_entry_len(k.len, vo, cs) != e1 - e0) continue;
        uint8_t* p = P.entries + e0;
        if (k.len) {
            *p++ = 0x0A;  // field 1, wire type 2
            p = pb_put_varint(p, k.len);
            for (uint64_t b = 0; b < k.len; b++) p[b] = k.p[b];
            p += k.len;
        }
        if (vo) {
            *p++ = 0x10;  // field 2, varint
            p = pb_put_varint(p, vo);
        }
        if (cs) {
            *p++ = 0x18;  // field 3, varint
            p = pb_put_varint(p, cs);
        }
    }
}

hipError_t launch_merge_plan(const MergeParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_merge_init, dim3(1), dim3(64), 0, s, P.result);
    if (P.N) {
        hipLaunchKernelGGL(k_merge_keys, dim3(grid_for(P.N, 256, kMergeGridCap)), dim3(256), 0, s, P);
        hipLaunchKernelGGL(k_merge_rank, dim3(grid_for(P.N, 256, kMergeGridCap)), dim3(256), 0, s, P);
    }
    return hipGetLastError();
}

hipError_t launch_merge_gather(const GatherParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_flags, dim3(grid_for(P.N + 1, 256, kMergeGridCap)), dim3(256), 0, s, P);
    hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.opos, P.N, s);
    if (e != hipSuccess) return e;
    if (P.N) hipLaunchKernelGGL(k_gather_select, dim3(grid_for(P.N, 256, kMergeGridCap)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_gather_pad, dim3(grid_for(P.n_out + 1, 256, kMergeGridCap)), dim3(256), 0, s, P);
    e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.val_off, P.n_out, s);
    if (e != hipSuccess) return e;
    if (P.n_out) launch_short_long(k_gather_copy<16, false>, k_gather_copy<64, true>, P.n_out, P, s);
    return hipGetLastError();
}

hipError_t launch_index_entries(const EntryParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_entry_len, dim3(grid_for(P.n_out + 1, 256, kMergeGridCap)), dim3(256), 0, s, P);
    hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.ent_off, P.n_out, s);
    if (e != hipSuccess) return e;
    if (P.n_out) hipLaunchKernelGGL(k_entry_write, dim3(grid_for(P.n_out, 256, kMergeGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

}  // namespace rio
