// rio_walops.hip — WAL recovery on the device: the WalMutation records of decoded WAL files become the op
// log a memstore flush takes. Replaces the host loop of replayAndSetupWriteAheadLog (simpledb/recovery.go:
// 208-240): proto.Unmarshal of every record into a WalMutation, then memStore.Upsert / Tombstone. Input: S
// decoded files as rio_device_decode leaves them in HBM (rio_wal_segment), in replay order; output: the
// arrays of a rio_ops_view (rio_sst_flush_plan, rio_flush.hip).
//
// Plan (rio_wal_ops_plan):
//   k_wal_parse    one lane per record over the concatenation of the segments; the lane finds its segment by
//                  a search over the record-count prefix, clamps the record's range to the segment's arena
//                  (RIO_WAL_BAD_RANGE when the clamp changed it), parses it (pb_wal_mutation_t, rio_pb.h) and
//                  applies the switch of recovery.go:224-237: kind, key range, value range; the scan inputs
//                  (is-op, key length, value length); the longest key and the smallest refused record with its
//                  class (LDS atomics per round, then one global atomic per block and round)
//   3 exclusive scans (hipcub::DeviceScan) over N + 1 items: op number, key offset, value offset of every
//                  record; item N holds the totals
//   k_wal_result   the result block
// Gather (rio_wal_ops_gather):
//   k_wal_offsets  one lane per record: key_off / val_off / flags / op_rec of its op, the final offsets
//   k_wal_copy<G, kLong>  G lanes per record (16 for items under kLongItem bytes, a wave for the others;
//                  a record's key and value each go to the instantiation of their length), copied with
//                  copy_item (rio_seg_copy.h); nothing is read or written outside the item. A group loads
//                  all of a record's bookkeeping words at once and has two records in flight. The value
//                  copy is the bandwidth path: every value byte is read once and written once.
// Every record, segment and op number read back from a buffer is clamped, every source range is clamped to
// its segment's arena again in the gather, and every store is checked against its capacity: a wrong input
// gives RIO_WAL_BAD_RANGE or wrong bytes, never an out-of-range access.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_pb.h"
#include "rio_seg_copy.h"

namespace rio {

namespace {

static_assert(kPbWalBadProto == RIO_WAL_BAD_PROTO && kPbWalBadUtf8 == RIO_WAL_BAD_UTF8, "parser classes are the ABI's");

// 256 CUs x 4 blocks of 256 lanes: longer logs go round the grid-stride loops again
constexpr uint64_t kWalGridCap = 1024;
// the shared copy grid and threshold (rio_seg_copy.h) under this file's own names: a reader of this
// file alone (a test that sizes its cases by them) finds the figures here, and the build fails if they part
constexpr uint64_t kWalCopyGridCap = 4096;
constexpr uint64_t kWalLongItem = 1024;
static_assert(kWalCopyGridCap == kCopyGridCap && kWalLongItem == kLongItem, "the shared copy constants");

// segment of record g: the last s with base[s] <= g (base[S] = N > g; empty segments repeat a base, the
// last of equal bases is the one that holds the record)
__device__ __forceinline__ uint32_t seg_of(const uint64_t* base, uint32_t S, uint64_t g) {
    uint32_t lo = 0, hi = S;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ void k_wal_init(WalParams P) {
    if (threadIdx.x < RIO_WAL_RESULT_WORDS) P.result[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        P.meta[0] = ~0ull;
        P.meta[1] = 0;
    }
}

__global__ void __launch_bounds__(256) k_wal_parse(WalParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // whole blocks iterate together for the barriers; item N is the scans' total slot
    __shared__ unsigned long long s_bad, s_max;
    const uint64_t rounds = (P.N + 1 + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t g = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (threadIdx.x == 0) {
            s_bad = ~0ull;
            s_max = 0;
        }
        __syncthreads();
        if (g < P.N) {
            const uint32_t s = seg_of(P.base, P.S, g);
            const rio_wal_segment& seg = P.segs[s];
            uint64_t i = g - P.base[s];
            uint32_t bad = 0;
            uint8_t kind = kWalNoOp;
            uint64_t ko = 0, kl = 0, vo = 0, vl = 0;
            if (i >= seg.n) {  // the bases are the segments' own counts: unreachable, but nothing is read then
                bad = RIO_WAL_BAD_RANGE;
            } else {
                const uint64_t o0 = seg.out_off[i], o1 = seg.out_off[i + 1];
                const uint64_t b = umin(o0, seg.out_bytes), e = umin(umax(o1, b), seg.out_bytes);
                if (b != o0 || e != o1) {
                    bad = RIO_WAL_BAD_RANGE;
                } else if (!(seg.flags[i] & RIO_FLAG_NIL) && e > b) {
                    RawBytes src{seg.out};
                    PbWalMutation m;
                    bad = pb_wal_mutation_t(src, b, e - b, m);
                    if (!bad && m.member == 1) {
                        kind = kWalUpsert;
                        if (m.kb_len) {
                            ko = b + m.kb_off, kl = m.kb_len;
                            vo = b + m.vb_off, vl = m.vb_len;
                            if (!vl) bad = RIO_WAL_BAD_VALUE_NIL;
                        } else {
                            ko = b + m.key_off, kl = m.key_len;
                            vo = b + m.val_off, vl = m.val_len;
                        }
                    } else if (!bad && m.member == 2) {
                        kind = kWalTombstone;
                        if (m.kb_len) ko = b + m.kb_off, kl = m.kb_len;
                        else ko = b + m.key_off, kl = m.key_len;
                    }
                }
            }
            if (bad) {
                kind = kWalNoOp;
                ko = kl = vo = vl = 0;
                atomicMin(&s_bad, (unsigned long long)(g << 3 | bad));
            }
            P.rec[g] = (uint32_t)kind | s << 8;
            P.koff[g] = ko;
            P.voff[g] = vo;
            P.klen[g] = kl;
            P.vlen[g] = vl;
            P.isop[g] = kind != kWalNoOp;
            if (kl) atomicMax(&s_max, (unsigned long long)kl);
        } else if (g == P.N) {
            P.klen[g] = P.vlen[g] = P.isop[g] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (s_bad != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&P.meta[0]), s_bad);
            if (s_max) atomicMax(reinterpret_cast<unsigned long long*>(&P.meta[1]), s_max);
        }
        __syncthreads();
    }
}

__global__ void k_wal_result(WalParams P) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t bad = P.meta[0];
    P.result[RIO_WAL_R_N_RECORDS] = P.N;
    P.result[RIO_WAL_R_N_OPS] = P.opos[P.N];
    P.result[RIO_WAL_R_KEY_BYTES] = P.kdst[P.N];
    P.result[RIO_WAL_R_VALUE_BYTES] = P.vdst[P.N];
    P.result[RIO_WAL_R_MAX_KEY_LEN] = P.meta[1];
    P.result[RIO_WAL_R_FIRST_BAD] = bad == ~0ull ? ~0ull : bad >> 3;
    P.result[RIO_WAL_R_BAD_CLASS] = bad == ~0ull ? 0 : bad & 7;
    P.result[7] = 0;
}

// op j's offsets, flag and source record; positions past the plan's count (a caller's n_ops larger than
// it) hold empty tombstones
__global__ void __launch_bounds__(256) k_wal_offsets(WalParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t have = P.opos[P.N], kend = P.kdst[P.N], vend = P.vdst[P.N];
    for (uint64_t g = t0; g < P.N; g += stride) {
        const uint32_t kind = P.rec[g] & 0xFFu;
        if (kind == kWalNoOp) continue;
        const uint64_t j = P.opos[g];
        if (j > P.n_ops) continue;  // a caller's n_ops smaller than the plan's: op n_ops only ends op n_ops - 1
        P.key_off[j] = P.kdst[g];
        P.val_off[j] = P.vdst[g];
        if (j < P.n_ops) {
            P.flags[j] = kind == kWalTombstone ? RIO_FLAG_NIL : 0;
            if (P.op_rec) P.op_rec[j] = g;
        }
    }
    for (uint64_t j = have + t0; j <= P.n_ops; j += stride) {
        P.key_off[j] = kend;
        P.val_off[j] = vend;
        if (j < P.n_ops) {
            P.flags[j] = RIO_FLAG_NIL;
            if (P.op_rec) P.op_rec[j] = ~0ull;
        }
    }
}

// record g's key and value as this instantiation's items (kLong = false: items shorter than kLongItem; true:
// the others). Every word of the record is loaded before the first is looked at, so the loads are in flight
// together; the segment and op numbers are clamped, the source ranges clamped to the segment's arena again (the
// scanned lengths are the ranges the plan checked), the destinations checked against their caps.
template <bool kLong>
__device__ __forceinline__ void wal_items(const WalParams& P, uint64_t g, CopyItem& k, CopyItem& v) {
    const uint32_t rec = P.rec[g];
    const uint64_t kd0 = P.kdst[g], kd1 = P.kdst[g + 1], vd0 = P.vdst[g], vd1 = P.vdst[g + 1];
    const uint64_t j = P.opos[g], ko = P.koff[g], vo = P.voff[g];
    k.len = v.len = 0;
    const uint32_t kind = rec & 0xFFu, sg = rec >> 8;
    if (kind == kWalNoOp || sg >= P.S || j >= P.n_ops) return;
    const rio_wal_segment& seg = P.segs[sg];
    const uint64_t ob = seg.out_bytes;
    const uint64_t kl = kd1 - kd0, vl = vd1 - vd0;
    if (kd1 > kd0 && (kl >= kLongItem) == kLong && kd1 <= P.keys_cap && ko <= ob && kl <= ob - ko)
        k = CopyItem{seg.out + ko, P.keys + kd0, kl};
    if (kind == kWalUpsert && vd1 > vd0 && (vl >= kLongItem) == kLong && vd1 <= P.values_cap && vo <= ob && vl <= ob - vo)
        v = CopyItem{seg.out + vo, P.values + vd0, vl};
}

template <uint32_t G>
__device__ __forceinline__ void wal_copy_item(const CopyItem& it, uint32_t lane) {
    if (it.len) copy_item<G>(it.d, it.s, it.len, lane);
}

// G lanes per record, two records per round so that one's bookkeeping loads overlap the other's copy
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_wal_copy(WalParams P) {
    const uint32_t lane = threadIdx.x % G;
    const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / G;
    for (uint64_t g = grp; g < P.N; g += 2 * ngrp) {
        CopyItem k0, v0, k1, v1;
        wal_items<kLong>(P, g, k0, v0);
        k1.len = v1.len = 0;
        if (g + ngrp < P.N) wal_items<kLong>(P, g + ngrp, k1, v1);
        wal_copy_item<G>(k0, lane);
        wal_copy_item<G>(v0, lane);
        wal_copy_item<G>(k1, lane);
        wal_copy_item<G>(v1, lane);
    }
}

hipError_t launch_wal_plan(const WalParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_wal_init, dim3(1), dim3(64), 0, s, P);
    hipLaunchKernelGGL(k_wal_parse, dim3(grid_for(P.N + 1, 256, kWalGridCap)), dim3(256), 0, s, P);
    const uint64_t* in[3] = {P.isop, P.klen, P.vlen};
    uint64_t* out[3] = {P.opos, P.kdst, P.vdst};
    for (int k = 0; k < 3; k++) {
        const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, in[k], out[k], P.N, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_wal_result, dim3(1), dim3(64), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_wal_gather(const WalParams& P, hipStream_t s) {
    hipLaunchKernelGGL(k_wal_offsets, dim3(grid_for(std::max(P.N, P.n_ops) + 1, 256, kWalGridCap)), dim3(256), 0, s, P);
    if (P.N && P.n_ops) launch_short_long(k_wal_copy<16, false>, k_wal_copy<64, true>, P.N, P, s);
    return hipGetLastError();
}

}  // namespace rio
