// rio_db.hip — the combined read of a batch of DB.GetBytes calls (simpledb/db.go:197-242): the table stack's
// answer (rio_sst_stack_lookup's source words) and the memstores' (rio_mem_lookup's) to a status byte, a value
// length and the value's bytes per query.
//
//   k_db_value_len      one lane per query: the table's status and length by k_stack_value_len's rules
//                       (table_status, rio_sst_keys.h), then db.go's rules in order: the table's read error first
//                       (:212-218), a memstore's value (:240-241, an empty one too), a memstore's tombstone
//                       (:231-234), the table's non-empty value (:228-229), else not found; the scan's input
//   k_db_value_copy<G>  G lanes per value (16 under kLongItem bytes, a wave for the others): copy_ranges
//                       (rio_seg_copy.h) from the op log's value arena (RIO_GET_MEM_VALUE) or the table's data
//                       arena (RIO_GET_VALUE)
// Every store, op, table and entry number read from a buffer is clamped (mem_op_of, entry_of), every range to its
// arena, every store is checked against values_cap: a wrong input gives RIO_GET_NOT_FOUND or wrong bytes, never an
// out-of-range access.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_seg_copy.h"
#include "rio_ops_keys.h"
#include "rio_sst_keys.h"

namespace rio {

namespace {
// 256 CUs x 8 blocks of 256 lanes: longer batches go round the grid-stride loops again
constexpr uint64_t kDbGridCap = 2048;
}  // namespace

// status and value length per query; position n holds the scan's last input, 0
__global__ void __launch_bounds__(256) k_db_value_len(DbParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= P.n; i += stride) {
        uint64_t len = 0;
        if (i < P.n) {
            uint64_t tlen = 0;
            uint32_t ts = RIO_GET_NOT_FOUND;
            if (P.tab_src && P.T) table_status(P.views, P.stored, P.T, P.check_crc, P.tab_src[i], ts, tlen);
            const rio_mem_index* I;
            uint64_t op;
            const bool in_mem = mem_op_of(P.i0, P.i1, P.n_idx, P.mem_src[i], I, op);
            uint32_t status = RIO_GET_NOT_FOUND;
            if (ts == RIO_GET_HOST) {
                status = RIO_GET_HOST;
            } else if (in_mem) {
                if (!(I->ops.flags[op] & RIO_FLAG_NIL)) {
                    uint64_t vb, ve;
                    value_range(I->ops, op, vb, ve);
                    len = ve - vb;
                    status = RIO_GET_MEM_VALUE;
                }
            } else if (ts == RIO_GET_VALUE && tlen > 0) {
                len = tlen;
                status = RIO_GET_VALUE;
            }
            P.status[i] = (uint8_t)status;
        }
        P.tmp[i] = len;
    }
}

// G lanes per value. kLong = false: values shorter than kLongItem; true: the others.
template <uint32_t G, bool kLong>
__global__ void __launch_bounds__(256) k_db_value_copy(DbParams P) {
    copy_ranges<G, kLong>(P.n, P.val_off, P.values_cap, P.values, [&](uint64_t j, uint64_t len) __attribute__((always_inline)) -> const uint8_t* {
        const uint32_t status = P.status[j];
        uint64_t vb, ve;
        if (status == RIO_GET_MEM_VALUE) {
            const rio_mem_index* I;
            uint64_t op;
            if (!mem_op_of(P.i0, P.i1, P.n_idx, P.mem_src[j], I, op)) return nullptr;
            value_range(I->ops, op, vb, ve);
            return ve - vb == len ? I->ops.values + vb : nullptr;
        }
        if (status == RIO_GET_VALUE && P.tab_src) {
            const rio_sst_view* v;
            uint64_t i;
            if (!entry_of(P.views, P.T, P.tab_src[j], v, i)) return nullptr;
            value_at(*v, i, vb, ve);
            return ve - vb == len ? v->data + vb : nullptr;
        }
        return nullptr;
    });
}

hipError_t launch_db_value_plan(const DbParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_db_value_len, dim3(grid_for(P.n + 1, 256, kDbGridCap)), dim3(256), 0, s, P);
    const hipError_t e = launch_offsets_scan(cub_tmp, cub_bytes, P.tmp, P.val_off, P.n, s);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_db_value_copy(const DbParams& P, hipStream_t s) {
    launch_short_long(k_db_value_copy<16, false>, k_db_value_copy<64, true>, P.n, P, s);
    return hipGetLastError();
}

}  // namespace rio
