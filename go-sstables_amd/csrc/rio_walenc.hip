// rio_walenc.hip — batched writes on the device: an op log becomes the WalMutation records of a WAL file. Replaces
// the per-mutation proto.Marshal of db.PutBytes / db.DeleteBytes (simpledb/db.go:258-265, :312-318), the inverse of
// k_wal_parse (rio_walops.hip). Input: a rio_ops_view as rio_sst_flush_plan takes it; output: a record arena and
// its offsets in the layout rio_device_encode frames into a v4 recordio image.
//
// Record i (deterministic field order, proto3 empty fields omitted, minimal varints, the oneof member always there):
//   upsert  0A varint(body)  [1A varint(klen) key]  [22 varint(vlen) value]
//   delete  12 varint(body)  [12 varint(klen) key]                          (the value range is not read)
//
// rio_wal_ops_encode:
//   k_walenc_init    the meta words
//   k_walenc_len     one lane per op: the key and value ranges clamped to their arenas (RIO_WAL_BAD_RANGE when the
//                    clamp changed one), the record's length as scan input (item n = 0), the counts, the longest
//                    key and the smallest refused op (LDS atomics per round, then one global atomic per block,
//                    round and word)
//   1 exclusive scan (hipcub::DeviceScan) over n + 1 items into the caller's rec_off; item n is the arena length
//   k_walenc_result  the result block
//   k_walenc_write<G, kLong>  G lanes per record (16 for items under kLongItem bytes, a wave for the others; a
//                    record's key and value each go to the instantiation of their length). The instantiation of the
//                    key's length writes the record's header bytes (at most 33, in two pieces: before the key and
//                    before the value) from one lane with plain byte stores; the group copies with copy_item
//                    (rio_seg_copy.h). Two records in flight per group, as k_wal_copy.
// Every offset read back from a buffer is clamped to its arena again in the write kernel, a record is written only
// when its scanned range equals the length computed from the clamped ranges and ends inside records_cap: a wrong
// input gives RIO_WAL_BAD_RANGE or unwritten records, never an out-of-range access.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"

namespace rio {

namespace {

// 256 CUs x 4 blocks of 256 lanes: longer logs go round the grid-stride loop again
constexpr uint64_t kWalEncGridCap = 1024;
// the shared copy grid and threshold (rio_seg_copy.h) under this file's own names: a reader of this
// file alone (a test that sizes its cases by them) finds the figures here, and the build fails if they part
constexpr uint64_t kWalEncCopyGridCap = 4096;
constexpr uint64_t kWalEncLongItem = 1024;
static_assert(kWalEncCopyGridCap == kCopyGridCap && kWalEncLongItem == kLongItem, "the shared copy constants");

constexpr uint32_t kMetaBad = 0, kMetaMaxKey = 1, kMetaUpserts = 2, kMetaDeletes = 3;

// a length-delimited field: tag, length, payload; nothing for an empty payload (proto3)
__device__ __forceinline__ uint64_t field_len(uint64_t payload) {
    return payload ? 1 + pb_varint_len(payload) + payload : 0;
}

// op g of the log: its clamped key and value ranges and what its record looks like
struct EncOp {
    uint64_t ko, kl, vo, vl;  // key and value range; vl = 0 for a delete
    uint64_t body, len;       // the member message's length, the record's
    bool del, bad;
};

__device__ __forceinline__ EncOp enc_op(const rio_ops_view& v, uint64_t g) {
    const uint64_t k0 = v.key_off[g], k1 = v.key_off[g + 1], v0 = v.val_off[g], v1 = v.val_off[g + 1];
    const uint8_t fl = v.flags[g];
    EncOp o;
    const uint64_t kb = umin(k0, v.key_bytes), ke = umin(umax(k1, kb), v.key_bytes);
    const uint64_t vb = umin(v0, v.value_bytes), ve = umin(umax(v1, vb), v.value_bytes);
    o.bad = kb != k0 || ke != k1 || vb != v0 || ve != v1;
    o.del = fl & RIO_FLAG_NIL;
    o.ko = kb, o.kl = ke - kb;
    o.vo = vb, o.vl = o.del ? 0 : ve - vb;
    o.body = field_len(o.kl) + field_len(o.vl);
    o.len = 1 + pb_varint_len(o.body) + o.body;
    return o;
}

}  // namespace

__global__ void k_walenc_init(WalEncParams P) {
    if (threadIdx.x < 4) P.meta[threadIdx.x] = threadIdx.x == kMetaBad ? ~0ull : 0;
}

__global__ void __launch_bounds__(256) k_walenc_len(WalEncParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n = P.ops.n;
    // whole blocks iterate together for the barriers; item n is the scan's total slot
    __shared__ unsigned long long s_bad, s_max;
    __shared__ unsigned int s_up, s_del;
    const uint64_t rounds = (n + 1 + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t g = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (threadIdx.x == 0) {
            s_bad = ~0ull;
            s_max = 0;
            s_up = s_del = 0;
        }
        __syncthreads();
        if (g < n) {
            const EncOp o = enc_op(P.ops, g);
            if (o.bad) {
                P.len[g] = 0;
                atomicMin(&s_bad, (unsigned long long)(g << 3 | RIO_WAL_BAD_RANGE));
            } else {
                P.len[g] = o.len;
                atomicAdd(o.del ? &s_del : &s_up, 1u);
                if (o.kl) atomicMax(&s_max, (unsigned long long)o.kl);
            }
        } else if (g == n) {
            P.len[g] = 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long* m = reinterpret_cast<unsigned long long*>(P.meta);
            if (s_bad != ~0ull) atomicMin(&m[kMetaBad], s_bad);
            if (s_max) atomicMax(&m[kMetaMaxKey], s_max);
            if (s_up) atomicAdd(&m[kMetaUpserts], (unsigned long long)s_up);
            if (s_del) atomicAdd(&m[kMetaDeletes], (unsigned long long)s_del);
        }
        __syncthreads();
    }
}

__global__ void k_walenc_result(WalEncParams P) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t bad = P.meta[kMetaBad];
    P.result[RIO_WALENC_R_N_RECORDS] = P.ops.n;
    P.result[RIO_WALENC_R_BYTES] = P.rec_off[P.ops.n];
    P.result[RIO_WALENC_R_N_UPSERTS] = P.meta[kMetaUpserts];
    P.result[RIO_WALENC_R_N_DELETES] = P.meta[kMetaDeletes];
    P.result[RIO_WALENC_R_MAX_KEY_LEN] = P.meta[kMetaMaxKey];
    P.result[RIO_WALENC_R_FIRST_BAD] = bad == ~0ull ? ~0ull : bad >> 3;
    P.result[RIO_WALENC_R_BAD_CLASS] = bad == ~0ull ? 0 : bad & 7;
    P.result[7] = 0;
}

namespace {

// what this instantiation does for record g: its items, and the header when it is the header's writer
struct EncRec {
    CopyItem k, v;
    uint8_t* d;  // the record's first byte when this instantiation writes the header, else null
    uint64_t body, kl, vl;
    bool del;
};

// Every word of the record is loaded before the first is looked at. The ranges are clamped as in k_walenc_len;
// the record is taken only when the scan's range for it is the length those ranges give and lies inside the cap,
// so every store below falls inside [rec_off[g], rec_off[g + 1]) <= records_cap.
template <bool kLong>
__device__ __forceinline__ void enc_rec(const WalEncParams& P, uint64_t g, EncRec& R) {
    const uint64_t r0 = P.rec_off[g], r1 = P.rec_off[g + 1];
    const EncOp o = enc_op(P.ops, g);
    R.k.len = R.v.len = 0;
    R.d = nullptr;
    if (o.bad || r1 < r0 || r1 - r0 != o.len || r1 > P.records_cap) return;
    const uint64_t h1 = 1 + pb_varint_len(o.body) + (o.kl ? 1 + pb_varint_len(o.kl) : 0);  // up to the key's first byte
    const uint64_t h2 = o.vl ? 1 + pb_varint_len(o.vl) : 0;                              // between key and value
    uint8_t* d = P.records + r0;
    if ((o.kl >= kLongItem) == kLong) {  // the key's instantiation writes the header (an empty key: the short one)
        R.d = d;
        R.body = o.body, R.kl = o.kl, R.vl = o.vl, R.del = o.del;
        if (o.kl) R.k = CopyItem{P.ops.keys + o.ko, d + h1, o.kl};
    }
    if (o.vl && (o.vl >= kLongItem) == kLong) R.v = CopyItem{P.ops.values + o.vo, d + h1 + o.kl + h2, o.vl};
}

// the record's header bytes, by one lane: member tag and body length, the key's tag and length, and behind the
// key the value's tag and length
__device__ __forceinline__ void enc_header(const EncRec& R) {
    uint8_t* p = R.d;
    *p++ = R.del ? 0x12 : 0x0A;
    p = pb_put_varint(p, R.body);
    if (R.kl) {
        *p++ = R.del ? 0x12 : 0x1A;
        p = pb_put_varint(p, R.kl) + R.kl;
    }
    if (R.vl) {
        *p++ = 0x22;
        pb_put_varint(p, R.vl);
    }
}

template <uint32_t G>
__device__ __forceinline__ void enc_write(const EncRec& R, uint32_t lane) {
    if (R.d && lane == 0) enc_header(R);
    if (R.k.len) copy_item<G>(R.k.d, R.k.s, R.k.len, lane);
    if (R.v.len) copy_item<G>(R.v.d, R.v.s, R.v.len, lane);
}

}  // namespace

// G lanes per record, two records per round so that one's bookkeeping loads overlap the other's copy
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_walenc_write(WalEncParams P) {
    const uint32_t lane = threadIdx.x % G;
    const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t ngrp = ((uint64_t)gridDim.x * blockDim.x) / G;
    const uint64_t n = P.ops.n;
    for (uint64_t g = grp; g < n; g += 2 * ngrp) {
        EncRec a, b;
        enc_rec<kLong>(P, g, a);
        b.k.len = b.v.len = 0;
        b.d = nullptr;
        if (g + ngrp < n) enc_rec<kLong>(P, g + ngrp, b);
        enc_write<G>(a, lane);
        enc_write<G>(b, lane);
    }
}

hipError_t launch_walenc(const WalEncParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    const uint64_t n = P.ops.n;
    hipLaunchKernelGGL(k_walenc_init, dim3(1), dim3(64), 0, s, P);
    hipLaunchKernelGGL(k_walenc_len, dim3(grid_for(n + 1, 256, kWalEncGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.len, P.rec_off, n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_walenc_result, dim3(1), dim3(64), 0, s, P);
    if (n && P.records_cap) launch_short_long(k_walenc_write<16, false>, k_walenc_write<64, true>, n, P, s);
    return hipGetLastError();
}

}  // namespace rio
