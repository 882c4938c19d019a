// rio_crc64.h — CRC-64/ISO (hash/crc64 with crc64.ISO, what the SSTable writer stores per value,
// sstable_writer.go:120-124) on the device: the slice-by-8 table in LDS and the per-lane value loop.
// Shared by k_sst_validate (rio_sstable.hip) and k_flush_crc (rio_flush.hip). Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rio_dev_util.h"

namespace rio {

// CRC-64/ISO, reflected, slice-by-8: tab[k][i] = CRC of byte i followed by k zero bytes, so one
// 8-byte step is eight independent LDS lookups instead of eight dependent ones.
__device__ __forceinline__ uint64_t crc64_step8(const uint64_t (*tab)[256], uint64_t c, uint64_t w) {
    c ^= w;
    return tab[7][c & 0xFF] ^ tab[6][(c >> 8) & 0xFF] ^ tab[5][(c >> 16) & 0xFF] ^ tab[4][(c >> 24) & 0xFF] ^
           tab[3][(c >> 32) & 0xFF] ^ tab[2][(c >> 40) & 0xFF] ^ tab[1][(c >> 48) & 0xFF] ^ tab[0][c >> 56];
}

// fills the block's table (16 KiB of LDS); every thread of the block calls it, it ends with a barrier
__device__ __forceinline__ void crc64_build_table(uint64_t (*tab)[256]) {
    for (uint32_t k = threadIdx.x; k < 256; k += blockDim.x) {
        uint64_t c = k;
        for (int j = 0; j < 8; j++) c = (c >> 1) ^ (0xD800000000000000ull & (0ull - (c & 1ull)));
        tab[0][k] = c;
    }
    __syncthreads();
    for (int t = 1; t < 8; t++) {
        for (uint32_t k = threadIdx.x; k < 256; k += blockDim.x)
            tab[t][k] = (tab[t - 1][k] >> 8) ^ tab[0][tab[t - 1][k] & 0xFF];
        __syncthreads();
    }
}

// CRC-64/ISO of v[0, len) by one lane; reads nothing outside the value
__device__ __forceinline__ uint64_t crc64_value(const uint64_t (*tab)[256], const uint8_t* v, uint64_t len) {
    uint64_t c = ~0ull, k = 0;
    // 64 bytes per iteration: four unaligned 16-byte loads in flight before the CRC steps
    for (; k + 64 <= len; k += 64) {
        uint4 w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = ldu16(v + k + 16 * q);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            c = crc64_step8(tab, c, ((uint64_t)w[q].y << 32) | w[q].x);
            c = crc64_step8(tab, c, ((uint64_t)w[q].w << 32) | w[q].z);
        }
    }
    for (; k + 16 <= len; k += 16) {
        const uint4 w = ldu16(v + k);
        c = crc64_step8(tab, c, ((uint64_t)w.y << 32) | w.x);
        c = crc64_step8(tab, c, ((uint64_t)w.w << 32) | w.z);
    }
    for (; k < len; k++) c = tab[0][(c ^ v[k]) & 0xFFu] ^ (c >> 8);
    return ~c;
}

}  // namespace rio
