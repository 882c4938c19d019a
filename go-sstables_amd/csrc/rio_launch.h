// rio_launch.h — every host-callable function a .hip file defines, declared once. Included by the .hip file
// that defines each function and by every caller, so the compiler checks the two sides against each other.
// Internal to librio.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_ext.h>  // launch_ev, for the .hip files
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "rio_device.h"

namespace rio {

// blocks for n items at per_block items a block: at least one, at most cap (the loops are grid-stride)
inline unsigned grid_for(uint64_t n, uint64_t per_block, uint64_t cap) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, cap));
}
// the same without a cap, for kernels that take one item per lane or group and do not loop
inline unsigned blocks_for(uint64_t n, unsigned bs) {
    uint64_t b = (n + bs - 1) / bs;
    return (unsigned)(b == 0 ? 1 : b);
}

// Stage timing rides on the kernels' own dispatches (hipExtLaunchKernelGGL's start / stop events): a separate
// hipEventRecord puts a marker packet between two kernels and cost ~5.6 us of idle queue each (rocprofv3 trace of a
// C2 step, profiles/r5/r5bh_ext_events_ab.txt); without events the launches are plain. For the .hip files (the host runtime launches no kernel).
#ifdef __HIPCC__
template <typename K, typename A>
inline void launch_ev(K kernel, dim3 g, dim3 b, hipStream_t s, hipEvent_t start, hipEvent_t stop, const A& P) {
    if (!start && !stop) {
        hipLaunchKernelGGL(kernel, g, b, 0, s, P);
        return;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
        hipExtLaunchKernelGGL(kernel, g, b, 0, s, start, stop, 0, P);
        return;
    }
    // under stream capture the events become record nodes around the kernel
    if (start) (void)hipEventRecord(start, s);
    hipLaunchKernelGGL(kernel, g, b, 0, s, P);
    if (stop) (void)hipEventRecord(stop, s);
}
#endif

// rio_walk.hip: the chunk walk, wave or lane by P.walk_lane (start / stop: the stage events, either may be null)
void launch_walk(const FrameParams& P, hipStream_t s, hipEvent_t start, hipEvent_t stop);
// rio_chunk_scan.hip: the chunk-summary scan, also run by the gzip and lzw redo rounds (stop: may be null)
void launch_chunk_scan(const FrameParams& P, hipStream_t s, hipEvent_t stop);
// rio_place.hip: the decode pipeline's launch sequence (framing, placement and the decoders' driver)
hipError_t launch_phase_a(const FrameParams& P, hipStream_t s, hipEvent_t* ev);
hipError_t launch_frame(const FrameParams& P, hipStream_t s, hipEvent_t* ev);
hipError_t launch_frame_ev(const FrameParams& P, hipStream_t s, hipEvent_t walk_start, hipEvent_t walk_stop,
                           hipEvent_t scan_stop);
hipError_t launch_phase_b(const FrameParams& P, hipStream_t s, hipEvent_t* ev, hipEvent_t done = nullptr);
hipError_t launch_phase_b_batch(const FrameBatch& B, hipStream_t s, hipEvent_t* ev, hipEvent_t done = nullptr);
// rio_seek.hip: single-record decode, the SeekNext map, DiskKeyIndex lookups
hipError_t launch_read_at(const uint8_t* f, uint64_t len, uint64_t off, uint8_t* out, uint64_t out_cap,
                          ReadAtResult* res, hipStream_t s);
hipError_t launch_seek_next(const uint8_t* f, uint64_t len, uint64_t off, uint64_t seek_len, uint8_t* out,
                            uint64_t out_cap, ReadAtResult* res, uint64_t* rec_off, hipStream_t s);
// the batch of ReadNextAt queries: the hits and offsets; the uncompressed copy (with the capacity rule); rio_snappy.hip:
// the Snappy copy (after launch_read_at_copy: it reads the rule's marks)
hipError_t launch_read_at_plan(const ReadAtParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_read_at_copy(const ReadAtParams& P, hipStream_t s);
hipError_t launch_read_at_snappy(const ReadAtParams& P, hipStream_t s);
int build_seek_map(const uint8_t* f, uint64_t len, const uint64_t* rec_off, const uint8_t* flags, uint64_t n,
                   std::vector<uint64_t>& P, std::vector<uint64_t>& R, hipStream_t s);
hipError_t launch_index_search(const uint8_t* f, uint64_t len, uint64_t seek_len, const uint8_t* keys,
                               const uint64_t* key_off, uint64_t nq, const uint32_t* perm, rio_index_hit* hits,
                               hipStream_t s);
hipError_t launch_index_search_view(const uint8_t* out, const uint64_t* out_off, const uint8_t* flags, uint64_t n,
                                    const uint64_t* P, uint64_t K, const uint64_t* R, uint64_t len, const uint8_t* keys,
                                    const uint64_t* key_off, uint64_t nq, const uint32_t* perm, rio_index_hit* hits,
                                    hipStream_t s);
// rio_snappy.hip, rio_gzip.hip, rio_lzw.hip: the codecs (called by rio_place.hip)
hipError_t launch_snappy_decode(const FrameParams& P, hipStream_t s, bool main);
hipError_t launch_snappy_batch(const FrameBatch& B, hipStream_t s);
hipError_t launch_gzip_decode(const FrameParams& P, hipStream_t s);
hipError_t launch_gzip_resize(const FrameParams& P, hipStream_t s);
hipError_t launch_lzw_decode(const FrameParams& P, hipStream_t s);
hipError_t launch_lzw_resize(const FrameParams& P, hipStream_t s);
// rio_sort.hip
size_t key_sort_tmp_bytes(uint64_t n);
hipError_t launch_key_sort(const uint8_t* keys, const uint64_t* key_off, uint64_t n, uint64_t* pfx_in, uint64_t* pfx_out,
                           uint32_t* idx_in, uint32_t* perm, void* tmp, size_t tmp_bytes, hipStream_t s);
// rio_sstable.hip
hipError_t launch_sst_index(const uint8_t* arena, const uint64_t* off, uint64_t n, uint64_t* key_off,
                            uint64_t* key_len, uint64_t* value_off, uint64_t* checksum, uint64_t* result,
                            hipStream_t s);
hipError_t launch_sst_validate(const uint8_t* data, const uint64_t* data_off, const uint64_t* data_rec_off,
                               uint64_t n_data, const uint64_t* value_off, const uint64_t* checksum,
                               uint64_t n_index, uint64_t* crc_out, uint64_t* result, hipStream_t s,
                               const uint64_t* view = nullptr);
hipError_t launch_sst_data_entry(const uint8_t* arena, const uint64_t* off, uint64_t n, uint64_t* view,
                                 uint64_t* result, hipStream_t s);
// rio_scan.hip: the exclusive sum of n + 1 lengths (the last one 0) into n + 1 offsets, and its scratch size
size_t scan_cub_bytes(uint64_t n);
hipError_t launch_offsets_scan(void* cub_tmp, size_t cub_bytes, const uint64_t* in, uint64_t* out, uint64_t n,
                               hipStream_t s);
// rio_compact.hip
hipError_t launch_merge_plan(const MergeParams& P, hipStream_t s);
hipError_t launch_merge_gather(const GatherParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_index_entries(const EntryParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
// rio_bloom.hip
hipError_t launch_bloom_add(const BloomParams& P, bool survivors, hipStream_t s);
hipError_t launch_bloom_contains(const BloomParams& P, hipStream_t s);
hipError_t launch_sst_key_prefixes(const rio_sst_view& v, uint64_t* pfx, hipStream_t s);
hipError_t launch_sst_lookup(const BloomParams& P, const LookupParams& Q, hipStream_t s);
// rio_stack.hip
hipError_t launch_stack_lookup(const StackParams& P, hipStream_t s);
hipError_t launch_stack_value_plan(const StackParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_stack_value_copy(const StackParams& P, hipStream_t s);
hipError_t launch_stack_bounds(const StackParams& P, hipStream_t s);
hipError_t launch_keys_gather(const KeysParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
// rio_flush.hip
size_t flush_cub_bytes(uint64_t n, uint32_t max_key_len);
hipError_t launch_flush_plan(const FlushParams& P, hipStream_t s, hipEvent_t* ev, uint32_t* n_stages,
                             bool with_crc = true);
// rio_memidx.hip
size_t mem_index_cub_bytes(uint64_t n);
hipError_t launch_mem_index(const MemBuildParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_mem_lookup(const MemLookupParams& P, hipStream_t s);
size_t mem_extend_cub_bytes(uint64_t t);
hipError_t launch_mem_extend(const MemExtendParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_ops_rebase(const OpsRebaseParams& P, hipStream_t s);
// rio_memsize.hip
size_t mem_size_cub_bytes(uint64_t n);
hipError_t launch_mem_size(const MemSizeParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
// rio_db.hip
hipError_t launch_db_value_plan(const DbParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_db_value_copy(const DbParams& P, hipStream_t s);
// rio_walops.hip
hipError_t launch_wal_plan(const WalParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
hipError_t launch_wal_gather(const WalParams& P, hipStream_t s);
// rio_walenc.hip
hipError_t launch_walenc(const WalEncParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
// rio_encode.hip
hipError_t launch_encode(const EncParams& P, void* cub_tmp, size_t cub_bytes, hipStream_t s);
uint64_t enc_scratch_bytes(uint64_t n, uint64_t bytes, uint32_t compression);
uint64_t enc_table_bytes();
size_t enc_cub_bytes(uint64_t n);

}  // namespace rio
