// rio_seg_copy.h — segmented copies: n items whose destination ranges are the exclusive scan of their lengths
// (off[j], off[j + 1]), copied by G lanes per item in two launches: 16 lanes per item under kLongItem bytes, a
// wave for the others. The copy of one item, the loop with its guards, the grid cap and the launch pair (grid_for: rio_launch.h), once
// for every kernel that copies this way (rio_compact, rio_stack, rio_db, rio_walops, rio_walenc). Included by
// .hip files only. Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_dev_util.h"
#include "rio_launch.h"

namespace rio {

constexpr uint64_t kLongItem = 1024;  // items from this length on are copied by a whole wave

// one thing to copy: len = 0 for nothing
struct CopyItem {
    const uint8_t* s;
    uint8_t* d;
    uint64_t len;
};

// len bytes from s to d by G lanes (lane = this lane's number among them): bytes up to the destination's next
// 16-byte boundary (the address decides), whole aligned 16-byte stores fed by unaligned 16-byte loads, then the
// tail bytes. Nothing is read outside [s, s + len) or written outside [d, d + len).
template <uint32_t G>
__device__ __forceinline__ void copy_item(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t lane) {
    const uint64_t head = umin((uint64_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15), len);
    if (lane < head) d[lane] = s[lane];
    const uint64_t body = (len - head) & ~15ull;
    for (uint64_t k = head + 16ull * lane; k < head + body; k += 16ull * G)
        *reinterpret_cast<uint4*>(d + k) = ldu16(s + k);
    const uint64_t t0 = head + body;
    if (t0 + lane < len && lane < 16) d[t0 + lane] = s[t0 + lane];
}

// The body of a copy kernel: item j goes to dst + [off[j], off[j + 1]), G lanes per item in a grid-stride loop.
// kLong = false takes the items shorter than kLongItem, true the others. An empty or reversed range, or one that
// ends past cap, is skipped. src(j, len) gives the item's first source byte, or null when the entry does not
// exist or its range is not len bytes long (the lengths scanned are these same ranges).
template <uint32_t G, bool kLong, typename Src>
__device__ __forceinline__ void copy_ranges(uint64_t n, const uint64_t* off, uint64_t cap, uint8_t* dst, Src src) {
    const uint32_t lane = threadIdx.x % G;
    const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / G;
    for (uint64_t j = grp; j < n; j += ngrp) {
        const uint64_t d0 = off[j], d1 = off[j + 1];
        if (d1 <= d0 || d1 > cap) continue;
        const uint64_t len = d1 - d0;
        if ((len >= kLongItem) != kLong) continue;
        const uint8_t* s = src(j, len);
        if (s) copy_item<G>(dst + d0, s, len, lane);
    }
}

// a block of 256 lanes takes 16 short or 4 long items per round
constexpr uint64_t kCopyGridCap = 4096;

// the two launches of a copy kernel k<G, kLong> over n items: the short items' instantiation, then the long ones'
template <typename Params>
inline void launch_short_long(void (*k16)(Params), void (*k64)(Params), uint64_t n, const Params& P, hipStream_t s) {
    hipLaunchKernelGGL(k16, dim3(grid_for(n, 16, kCopyGridCap)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k64, dim3(grid_for(n, 4, kCopyGridCap)), dim3(256), 0, s, P);
}

}  // namespace rio
