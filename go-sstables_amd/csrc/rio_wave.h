// rio_wave.h — wave-level helpers of the kernels (64-lane waves): prefix scans on DPP and on __shfl_up, group
// ballots, lane reads, the wave-local LDS fence. One copy of each, for the framing kernels and the codecs.
// Included by .hip files only. Internal to librio.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rio {

// Inclusive scan (sum, or max for kMax) within each 16-lane DPP row: row shifts, VALU latency instead of the LDS
// round trips of __shfl_up
template <bool kMax>
__device__ __forceinline__ uint32_t row_incl(uint32_t v) {
    auto op = [](uint32_t a, uint32_t b) { return kMax ? (a > b ? a : b) : a + b; };
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    return v;
}
// Wave-wide inclusive scan on DPP: the row scans, then row broadcasts 15 / 31
template <bool kMax>
__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
    auto op = [](uint32_t a, uint32_t b) { return kMax ? (a > b ? a : b) : a + b; };
    v = row_incl<kMax>(v);
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}
__device__ __forceinline__ uint32_t lane63(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

// Wave-wide exclusive prefix sum on __shfl_up (any integer width), and the wave's total
template <typename T>
__device__ __forceinline__ T wave_excl(T v, uint32_t lane, T& total) {
    T x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        x += lane >= d ? y : (T)0;
    }
    total = __shfl(x, 63, 64);
    return x - v;
}
template <typename T>
__device__ __forceinline__ T wave_excl(T v, uint32_t lane) {
    T total;
    return wave_excl(v, lane, total);
}

// exclusive prefix of 64-bit values and the wave total: 32-bit DPP when every value is below 2^26
// (64 of them sum below 2^32), else the shuffle scan
__device__ __forceinline__ uint64_t wave_excl_scan64(uint64_t v, uint32_t lane, uint64_t& total) {
    if (__all(v < (1ull << 26))) {
        const uint32_t x = wave_incl<false>((uint32_t)v);
        total = lane63(x);
        return x - (uint32_t)v;
    }
    return wave_excl(v, lane, total);
}

// The same within 16-lane groups (a wave's four DPP rows; lane = the lane within its group): exclusive prefix
// and the group's total
__device__ __forceinline__ uint64_t group16_excl_scan64(uint64_t v, uint32_t lane, uint64_t& total) {
    if (__all(v < (1ull << 26))) {
        const uint32_t x = row_incl<false>((uint32_t)v);
        total = (uint32_t)__shfl((int)x, 15, 16);
        return x - (uint32_t)v;
    }
    uint64_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 16; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 16);
        if (lane >= d) x += y;
    }
    total = __shfl(x, 15, 16);
    return x - v;
}

// a predicate's lanes within the caller's group of G lanes (G = 16 or 64), bit 0 = the group's lane 0
template <uint32_t G>
__device__ __forceinline__ uint64_t group_ballot(bool b) {
    const uint64_t m = __ballot(b);
    return G == 64 ? m : (m >> (threadIdx.x & 48u)) & 0xFFFFull;
}

// LDS written by some lanes of the wave, read by others: a wave-level fence and barrier, no workgroup barrier
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_ffs(uint64_t m) { return m ? (uint32_t)__builtin_ctzll(m) : 64u; }

// lane k's value for a wave-uniform k < 64: v_readlane into scalars (no LDS round trip of __shfl)
__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)k);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace rio
