// rio_bloom.hip — the bloom filter of a table and the point lookup of a loaded table on the device.
// Write side: SSTableStreamWriter's filter (sstables/sstable_writer.go:78-83 NewOptimal, :114-118 one Add per
// key, :150-154 WriteFile) for the tables the device writes. Read side: SSTableReader.Contains / Get
// (sstable_reader.go:49-77) over SliceKeyIndex (slice_key_index.go:19-35) for a batch of query keys.
//
// The filter is steakknife/bloomfilter's, its layout pinned by the reference's bloom.bf.gz fixtures: m bits in
// little-endian 64-bit words (bit i = bit i & 63 of word i >> 6), k random 64-bit hash keys. An element is the
// FNV-1 hash of the key (hash/fnv New64: h = basis; per byte h *= prime, then h ^= byte; not FNV-1a). Probe j is
// bit (h ^ hash_key[j]) mod m in full 64 bits: m may exceed 2^32, and plain % is exact. A 32-bit atomic OR on
// dword idx >> 5 writes the same memory as the file's 64-bit words (little-endian).
//
//   k_bloom_add<kSurvivors>  one lane per key: FNV-1, then k no-return atomic ORs. Keys come from an arena with
//                            offsets, or from the survivors of the context's last plan (d_out_src resolved through
//                            the plan's views, as k_entry_len finds its keys)
//   k_bloom_contains         one lane per key: the probes stop at the first clear bit; one byte per key
//   k_sst_key_prefixes       one lane per entry of a view: the 8-byte big-endian key prefix
//   k_sst_lookup             one lane per query: optional filter gate, lower bound over the prefixes (a byte
//                            compare only on equal prefixes), entry index on equality, else ~0
// The hash keys (k <= RIO_BLOOM_MAX_K) are staged in LDS once per block. Grid-stride loops of 256-lane blocks,
// at most kBloomGridCap blocks. Every key range is clamped to its arena and read inside it (8-byte loads where 8
// bytes are left in the arena, bytes otherwise); every entry index is clamped to its table: a wrong input gives
// wrong answers or ~0, never an out-of-range access.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {

// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loops again
constexpr uint64_t kBloomGridCap = 2048;
// key i of an arena with offsets: clamped to [0, key_bytes); room = bytes readable from its first byte
__device__ __forceinline__ const uint8_t* arena_key(const BloomParams& P, uint64_t i, uint64_t& len, uint64_t& room) {
    const uint64_t a = P.key_off[i], b = P.key_off[i + 1];
    const uint64_t off = umin(a, P.key_bytes);
    const uint64_t e = umin(umax(b, off), P.key_bytes);
    len = e - off;
    room = P.key_bytes - off;
    return P.keys + off;
}

__device__ __forceinline__ void load_hash_keys(uint64_t* s_hk, const rio_bloom_view& f) {
    if (threadIdx.x < umin(f.k, RIO_BLOOM_MAX_K)) s_hk[threadIdx.x] = f.hash_keys[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ void filter_add(const rio_bloom_view& f, const uint64_t* s_hk, uint64_t h) {
    uint32_t* words = reinterpret_cast<uint32_t*>(f.bits);
    const uint32_t k = umin(f.k, RIO_BLOOM_MAX_K);  // the host refuses a larger k; s_hk holds this many
    for (uint32_t j = 0; j < k; j++) {
        const uint64_t idx = (h ^ s_hk[j]) % f.m;  // < m: dword idx >> 5 lies inside 8 * ceil(m / 64) bytes
        atomicOr(&words[idx >> 5], 1u << (idx & 31));
    }
}

}  // namespace

template <bool kSurvivors>
__global__ void __launch_bounds__(256) k_bloom_add(BloomParams P) {
    __shared__ uint64_t s_hk[RIO_BLOOM_MAX_K];
    load_hash_keys(s_hk, P.f);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        const uint8_t* p;
        uint64_t len, room;
        if (kSurvivors) {
            const rio_sst_view* v;
            uint64_t e;
            if (!entry_of(P.views, P.T, P.out_src[i], v, e)) continue;  // a padded position: no key
            bool ok;
            const Key k = key_at(*v, e, ok);
            p = k.p;
            len = k.len;
            room = v->index_bytes - (uint64_t)(k.p - v->index);
        } else {
            p = arena_key(P, i, len, room);
        }
        filter_add(P.f, s_hk, fnv1(p, len, room));
    }
}

__global__ void __launch_bounds__(256) k_bloom_contains(BloomParams P) {
    __shared__ uint64_t s_hk[RIO_BLOOM_MAX_K];
    load_hash_keys(s_hk, P.f);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        uint64_t len, room;
        const uint8_t* p = arena_key(P, i, len, room);
        P.hit[i] = filter_contains(P.f, s_hk, fnv1(p, len, room)) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_sst_key_prefixes(rio_sst_view v, uint64_t* pfx) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < v.n; i += stride) {
        bool ok;
        pfx[i] = key_prefix(key_at(v, i, ok));
    }
}

__global__ void __launch_bounds__(256) k_sst_lookup(BloomParams P, LookupParams Q) {
    __shared__ uint64_t s_hk[RIO_BLOOM_MAX_K];
    const bool gate = P.f.bits != nullptr;  // uniform over the grid
    if (gate) load_hash_keys(s_hk, P.f);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += stride) {
        uint64_t len, room;
        const uint8_t* p = arena_key(P, i, len, room);
        uint64_t found = ~0ull;
        if (!gate || filter_contains(P.f, s_hk, fnv1(p, len, room))) {
            Key q{p, len, 0};
            q.pfx = key_prefix(q);
            const uint64_t lb = bound<false>(Q.v, Q.pfx, q);
            if (lb < Q.v.n && entry_cmp(Q.v, Q.pfx, lb, q) == 0) found = lb;
        }
        Q.entry[i] = found;
    }
}

hipError_t launch_bloom_add(const BloomParams& P, bool survivors, hipStream_t s) {
    if (survivors) hipLaunchKernelGGL(k_bloom_add<true>, dim3(grid_for(P.n, 256, kBloomGridCap)), dim3(256), 0, s, P);
    else hipLaunchKernelGGL(k_bloom_add<false>, dim3(grid_for(P.n, 256, kBloomGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_bloom_contains(const BloomParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_bloom_contains, dim3(grid_for(P.n, 256, kBloomGridCap)), dim3(256), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_sst_key_prefixes(const rio_sst_view& v, uint64_t* pfx, hipStream_t s) {
    hipLaunchKernelGGL(k_sst_key_prefixes, dim3(grid_for(v.n, 256, kBloomGridCap)), dim3(256), 0, s, v, pfx);
    return hipGetLastError();
}

hipError_t launch_sst_lookup(const BloomParams& P, const LookupParams& Q, hipStream_t s) {
    hipLaunchKernelGGL(k_sst_lookup, dim3(grid_for(P.n, 256, kBloomGridCap)), dim3(256), 0, s, P, Q);
    return hipGetLastError();
}

}  // namespace rio
