// rio_sstable.hip — device side of an SSTable's load, validation and full scan on top of the
// recordio decode (sstables/sstable_reader.go, sstable_iterator.go, slice_key_index.go).
//
// An SSTable is data.rio (values: one recordio record per value, Snappy by default,
// sstable_writer.go:50-56,219-220) + index.rio (one protobuf IndexEntry {key = 1, valueOffset = 2,
// checksum = 3} per record, sstables/proto/sstable.proto:5-9, uncompressed by default). Both files
// are decoded by the recordio path (rio_device_decode); these kernels work on the decoded arenas:
//
// k_sst_index    one lane per index record: proto.Unmarshal into a reset IndexEntry
//                (SliceKeyIndexLoader.Load, slice_key_index.go:91-131): wire format restated from
//                protowire (varints <= 10 bytes, field numbers 1 .. 2^29-1, last occurrence wins,
//                known fields with another wire type and unknown fields skipped, groups skipped to
//                their end tag). Outputs key (offset / length into the index arena), valueOffset,
//                checksum; the first malformed record is reported.
// k_sst_validate one lane per index entry: the value is the data record whose file offset is the
//                entry's valueOffset (MMapReader.ReadNextAt, sstable_reader.go:85-92) — record i
//                for every table the writer produced (valueOffset = the offset its data write
//                returned, sstable_writer.go:126-132) — then CRC-64/ISO of the value
//                (checksumValue, :240-248) against the stored checksum, 0 meaning "no checksum"
//                (:100-108). Outputs every entry's CRC-64, the first mismatching entry, and the
//                first entry not in the writer's layout (valueOffset is not data record i's offset:
//                the scan's positional pairing and validation would diverge; the adapter keeps the
//                reference reader).
// k_sst_data_entry one lane per data record of a v0 table (metadata version 0, sstable_reader.go:
//                303-314): proto.Unmarshal into a DataEntry {value = 1} (sstable.proto:12-14), as
//                MMapProtoReader.ReadNextAt / ProtoReader.ReadNext do for every value
//                (recordio/proto/mmap_proto_reader.go:12-24). Outputs the value's [begin, end) in the data
//                arena (kValueNil both for an absent field: value nil), the first malformed record.
//                k_sst_validate then hashes these ranges instead of the whole records.
#include <hip/hip_runtime.h>

#include "rio_crc64.h"
#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_launch.h"
#include "rio_pb.h"

namespace rio {


__global__ void __launch_bounds__(256) k_sst_index(const uint8_t* arena, const uint64_t* off, uint64_t n,
                                                   uint64_t* key_off, uint64_t* key_len, uint64_t* value_off,
                                                   uint64_t* checksum, unsigned long long* first_bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t base = off[i], len = off[i + 1] - base;
        const uint8_t* b = arena + base;
        uint64_t ko, kl, vo, cs;
        const bool ok = pb_index_entry(b, len, ko, kl, vo, cs);
        key_off[i] = base + ko;
        key_len[i] = kl;
        value_off[i] = vo;
        checksum[i] = cs;
        if (!ok) atomicMin(first_bad, (unsigned long long)i);
    }
}

__global__ void __launch_bounds__(256) k_sst_data_entry(const uint8_t* arena, const uint64_t* off, uint64_t n,
                                                        uint64_t* view, unsigned long long* first_bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint64_t base = off[j], len = off[j + 1] - base;
        RawBytes g{arena};
        bool present;
        uint64_t vo, vl;
        const bool ok = pb_data_entry_t(g, base, len, present, vo, vl);
        view[2 * j] = ok ? (present ? base + vo : RIO_VALUE_NIL) : RIO_VALUE_BAD;
        view[2 * j + 1] = ok ? (present ? base + vo + vl : RIO_VALUE_NIL) : RIO_VALUE_BAD;
        if (!ok) atomicMin(first_bad, (unsigned long long)j);
    }
}

// view == nullptr: the value of data record j is the whole record; else [view[2j], view[2j+1]) (v0
// DataEntry values; a nil or malformed one hashes as empty)
__global__ void __launch_bounds__(256) k_sst_validate(const uint8_t* data, const uint64_t* data_off,
                                                      const uint64_t* data_rec_off, uint64_t n_data,
                                                      const uint64_t* value_off, const uint64_t* checksum,
                                                      uint64_t n_index, uint64_t* crc_out,
                                                      unsigned long long* result, const uint64_t* view) {
    __shared__ uint64_t tab[8][256];  // 16 KiB
    crc64_build_table(tab);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_index; i += stride) {
        const uint64_t want = value_off[i];
        uint64_t j = i;
        if (!(i < n_data && data_rec_off[i] == want)) {
            // not the writer's layout (entry i <-> data record i): the full scan pairs entries and
            // records by position while validation follows valueOffset, so the device path hands
            // the table back; the search still gives validation its value
            uint64_t lo = 0, hi = n_data;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (data_rec_off[mid] < want) lo = mid + 1; else hi = mid;
            }
            if (lo >= n_data || data_rec_off[lo] != want) {
                crc_out[i] = 0;
                atomicMin(&result[1], (unsigned long long)i);
                continue;
            }
            j = lo;
            atomicMin(&result[1], (unsigned long long)i);
        }
        uint64_t vb = data_off[j], ve = data_off[j + 1];
        if (view) {
            vb = view[2 * j];
            ve = view[2 * j + 1];
            if (vb >= RIO_VALUE_BAD) vb = ve = 0;
        }
        const uint64_t c = crc64_value(tab, data + vb, ve - vb);
        crc_out[i] = c;
        if (checksum[i] != 0 && c != checksum[i]) atomicMin(&result[0], (unsigned long long)i);
    }
}

__global__ void k_sst_init(unsigned long long* r, int n) {
    if (threadIdx.x < (unsigned)n) r[threadIdx.x] = ~0ull;
}

hipError_t launch_sst_index(const uint8_t* arena, const uint64_t* off, uint64_t n, uint64_t* key_off,
                            uint64_t* key_len, uint64_t* value_off, uint64_t* checksum, uint64_t* result,
                            hipStream_t s) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
    hipLaunchKernelGGL(k_sst_init, dim3(1), dim3(64), 0, s, r, 1);
    const uint64_t blocks = (n + 255) / 256;
    if (n) hipLaunchKernelGGL(k_sst_index, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, arena, off,
                              n, key_off, key_len, value_off, checksum, r);
    return hipGetLastError();
}

hipError_t launch_sst_data_entry(const uint8_t* arena, const uint64_t* off, uint64_t n, uint64_t* view,
                                 uint64_t* result, hipStream_t s) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
    hipLaunchKernelGGL(k_sst_init, dim3(1), dim3(64), 0, s, r, 1);
    const uint64_t blocks = (n + 255) / 256;
    if (n)
        hipLaunchKernelGGL(k_sst_data_entry, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, arena, off,
                           n, view, r);
    return hipGetLastError();
}

hipError_t launch_sst_validate(const uint8_t* data, const uint64_t* data_off, const uint64_t* data_rec_off,
                               uint64_t n_data, const uint64_t* value_off, const uint64_t* checksum,
                               uint64_t n_index, uint64_t* crc_out, uint64_t* result, hipStream_t s,
                               const uint64_t* view) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
    hipLaunchKernelGGL(k_sst_init, dim3(1), dim3(64), 0, s, r, 2);
    const uint64_t blocks = (n_index + 255) / 256;
    if (n_index)
        hipLaunchKernelGGL(k_sst_validate, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, data,
                           data_off, data_rec_off, n_data, value_off, checksum, n_index, crc_out, r, view);
    return hipGetLastError();
}

}  // namespace rio
